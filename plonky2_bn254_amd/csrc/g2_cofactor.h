// The cofactor-clearing kernel for callers whose points are on the device already (map_to_g2.hip): defined in g2_cofactor.hip.
#pragma once
#include "ctx.h"

// k_g2_clear_cofactor on n points (d_points: n x 16 canonical words below p) on the context's stream, without waiting for it:
// d_images n x 16 words (zeros where the image is O), d_finite n bytes, *d_bad_idx (preset to UINT_MAX) lowered to the first point
// that is not on the twist curve.  n < UINT_MAX.
int bn254s_g2_clear_cofactor_device(bn254s_ctx* c, const u64* d_points, size_t n, u64* d_images, unsigned char* d_finite,
                                    unsigned* d_bad_idx);
