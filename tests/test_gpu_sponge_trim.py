"""k_leaf_hash with the sponge's trimmed last round: the last MDS layer of a permutation computes only the lanes that the next
absorb keeps (8..11 before a full chunk), that the digest reads (0..3 after the last chunk), or all twelve (before a ragged
chunk, which keeps some of lanes 0..7).  Column counts around the chunk size put every sequence of the three variants in
front of the oracle: coefficients, LDE and Merkle cap of PolynomialBatch::from_values, bit for bit.  2^16 rows give 2^17 leaves,
above the threshold of the cooperative kernels, so k_leaf_hash itself runs."""
import numpy as np
import pytest

from tests import oracle_lib

P = 2**64 - 2**32 + 1
pytestmark = pytest.mark.gpu
ROWS = 65536


def rand_field(rng, shape):
    v = rng.integers(0, 2**63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)
    return np.where(v >= np.uint64(P), v - np.uint64(P), v)


# 8: one full chunk (final variant only); 9: ragged (untrimmed, final); 16: next-full, final; 17 and 21: next-full, untrimmed,
# final (short and longer tail); 24: next-full twice, final
@pytest.mark.parametrize("ncols", [8, 9, 16, 17, 21, 24])
def test_commit_values_around_the_chunk_size(gpu_ctx, oracle, ncols):
    rng = np.random.default_rng(4000 + ncols)
    edge = np.array([0, 1, 2, P - 1, P - 2, 2**32 - 1, 2**32, 2**32 + 1, P - 2**32, 2**63, 2**48, 0xFFFFFFFE00000001,
                     0xFFFFFFFEFFFFFFFF, 0x00000001FFFFFFFF, 0xFFFF0000FFFF0001], dtype=np.uint64)
    vals = rand_field(rng, (ncols, ROWS))
    vals[1] = 0                                                   # an all-zero column
    vals[2, :] = np.uint64(P - 1)                                 # constant column at the top of the range
    vals[3] = edge[rng.integers(0, edge.size, size=ROWS)]         # mixtures of boundary values, one of them in the last chunk
    vals[ncols - 1] = edge[rng.integers(0, edge.size, size=ROWS)]
    c_ref, l_ref, cap_ref = oracle_lib.commit_values(oracle, vals)
    c, l, cap = gpu_ctx.commit_values(vals)
    assert np.array_equal(c, c_ref)
    assert np.array_equal(l, l_ref)
    assert np.array_equal(cap, cap_ref)
