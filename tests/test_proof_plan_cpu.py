"""The plan of a proof (csrc/proof_plan.hip, through bn254s_selftest_proof_plan; no GPU, no context): which workspace a proof of a
given kind and height gets, at the real thresholds, and the buffer sizes the workspace relies on.

The expected rows are worked out by hand from the formulas of the prover, with W / A = 781 / 456 (G1), 1295 / 906 (G2), 427 / 134
(Fq-exp), N rows and a device of 288 GiB = 309.2e9 bytes:
  plain layout    8 N (4 W + 4 A + max(W, A)) bytes; left for the compact one above 200e9
  compact layout  8 N (max(W, 2 A) + 3 W + A) bytes; left for the streaming one when it leaves less than 20e9 of the device
  G1 2^22: plain 8 * 2^22 * 5729 = 192.2e9 (stays);   G1 2^23: split level -> compact, 8 * 2^23 * 3711 = 249.0e9 (+ 20e9 fits)
  G2 2^21: plain 8 * 2^21 * 10099 = 169.4e9 (stays);  G2 2^22: plain 338.9e9 -> compact 8 * 2^22 * 6603 = 221.6e9 (fits)
  G2 2^23: compact 443.1e9 -> streaming;              Fq 2^23: compact 8 * 2^23 * 1842 = 123.6e9 (fits)"""
import pytest

import plonky2_bn254_amd as pk

G1, G2, FQ = 0, 1, 2
WIDTHS = {G1: (781, 456), G2: (1295, 906), FQ: (427, 134)}
POINT_WORDS = {G1: 8, G2: 16, FQ: 4}
DEV = 288 << 30
NQ, CH = 4, 16


@pytest.mark.parametrize("kind,n,dev,log_n,log_s,lowmem,stream", [
    (G1, 128, DEV, 16, 0, False, False),
    (G1, 8192, DEV, 22, 0, False, False),        # plain: 192 GB < 200 GB
    (G1, 16384, DEV, 23, 1, True, False),        # compact: 249 + 20 GB < 309 GB
    (G2, 4096, DEV, 21, 0, False, False),
    (G2, 8192, DEV, 22, 0, True, False),         # 339 GB plain -> compact
    (G2, 16384, DEV, 23, 1, True, True),         # 443 GB compact -> streaming
    (G2, 16384, 0, 23, 1, True, False),          # device size unknown: never streams on that account, still compact
    (FQ, 16384, DEV, 23, 1, True, False),
])
def test_workspace_choice_at_the_real_thresholds(kind, n, dev, log_n, log_s, lowmem, stream):
    p = pk.proof_plan(kind, n, dev)
    W, A = WIDTHS[kind]
    N = 1 << log_n
    assert (p["kind"], p["n"], p["W"], p["A"], p["point_words"]) == (kind, n, W, A, POINT_WORDS[kind])
    assert (p["N"], p["log_n"], p["log_s"], p["lowmem"], p["stream"]) == (N, log_n, log_s, int(lowmem), int(stream))
    assert (p["log_r"], p["R"], p["NH"], p["NSPL"]) == (log_n - 16 - log_s, 1 << (log_n - 16 - log_s), N >> log_s, 1 << log_s)
    assert p["in_words"] == n * (4 + 2 * POINT_WORDS[kind]) and p["words"]["in"] == p["in_words"] + 16


def test_smallest_proof_in_full():
    """G1, 128 instances: 2^16 rows, plain layout, arities [4, 4, 4]; every derived size from the word layout of the proof."""
    p = pk.proof_plan(G1, 128, DEV)
    nq = pk.default_params().num_queries
    W, A, N, M2 = 781, 456, 1 << 16, 1 << 17
    assert p["L"] == 3 and p["arities"] == [4, 4, 4]
    # per query: one row of each commitment + three paths of 17 - 4 digests; per layer a coset of 16 and a path to the cap
    assert p["wpq"] == (W + A + NQ) + 3 * 4 * 13 + (32 + 4 * 9) + (32 + 4 * 5) + (32 + 4 * 1)
    assert p["tree_words"] == 4 * (2 * M2 - 16)                           # levels of 2^17 .. 2^4 digests
    assert p["fri_words"] == 2 * (M2 + M2 // 16 + M2 // 256 + M2 // 4096)
    assert p["fri_tree_words"] == 4 * ((2 << 13) - 16 + (2 << 9) - 16 + (2 << 5) - 16)
    w = p["words"]
    assert (w["tvals"], w["tcoef"], w["tlde"]) == (W * N, W * N, W * M2)
    assert (w["avals"], w["acoef"], w["alde"]) == (A * N, A * N, A * M2)
    assert w["tmp"] == 3 * W * N                                          # [tmp | y0 | y1] of the fused commitment
    assert (w["ldechunk"], w["sponge"], w["win"]) == (0, 0, 0)
    assert w["comb"] == 6 * N + 6 * M2 and w["trees"] == 3 * p["tree_words"]
    assert w["quot"] == 3 * NQ * N + NQ * M2 + 7 * 2 * M2
    assert w["open"] == (W + A + NQ) * 5 + 4096                           # one block per polynomial, then the power tables
    assert (w["fri"], w["fritrees"], w["qout"]) == (p["fri_words"], p["fri_tree_words"], p["wpq"] * nq + 64)
    assert p["pinned_bytes"] == 8 * p["wpq"] * nq


def test_tall_plain_layout_has_one_transform_scratch():
    w = pk.proof_plan(G1, 8192, DEV)["words"]
    assert w["tmp"] == 781 << 22 and w["acoef"] == 456 << 22 and w["alde"] == 456 << 23


@pytest.mark.parametrize("kind,n,log_n,kw", [(G1, 16384, 23, {}), (G2, 8192, 22, {}), (G1, 150, 17, {"force_lowmem": True}),
                                             (FQ, 300, 18, {"force_split": True})])
def test_compact_workspace_aliasing(kind, n, log_n, kw):
    """The auxiliary LDE takes the memory of the dead trace values, the auxiliary commitment runs in place, the NTT works on one
    chunk of 16 columns (three of them under the split level)."""
    p = pk.proof_plan(kind, n, DEV, **kw)
    W, A = WIDTHS[kind]
    N = 1 << log_n
    w = p["words"]
    assert p["lowmem"] == 1 and p["stream"] == 0
    assert w["tvals"] == max(W * N, A * 2 * N)
    assert (w["acoef"], w["alde"]) == (0, 0) and w["avals"] == A * N and w["tlde"] == W * 2 * N
    assert w["tmp"] == (3 if p["log_s"] else 1) * CH * N
    assert (w["ldechunk"], w["sponge"], w["win"]) == (0, 0, 0)


@pytest.mark.parametrize("kind,n,log_n,kw,windows", [
    (G2, 16384, 23, {}, 2),
    (G1, 150, 17, {"force_stream": True, "stream_win_log": 15}, 4),
    (FQ, 300, 18, {"force_split": True, "force_stream": True, "stream_win_log": 16}, 4),
])
def test_streaming_workspace(kind, n, log_n, kw, windows):
    """No LDE has a buffer of its own: one chunk of 16 columns and the sponge states instead, the quotient in windows."""
    p = pk.proof_plan(kind, n, DEV, **kw)
    W, A = WIDTHS[kind]
    N = 1 << log_n
    nq = pk.default_params().num_queries
    w = p["words"]
    assert p["stream"] == 1 and p["lowmem"] == 1 and p["log_s"] == (1 if log_n == 23 or kw.get("force_split") else 0)
    assert p["N"] // p["BK"] == windows and p["BK"] == 1 << p["log_bk"] and p["WROWS"] == p["BK"] + 1
    assert (w["tlde"], w["alde"], w["acoef"]) == (0, 0, 0)
    assert (w["tvals"], w["tcoef"], w["avals"]) == (W * N, W * N, A * N)
    assert (w["ldechunk"], w["sponge"]) == (CH * 2 * N, 12 * 2 * N)
    assert w["win"] == (W + A) * p["WROWS"] + 3 * p["WROWS"] + (W + A) * nq
    assert w["quot"] == 3 * NQ * N + NQ * 2 * N + 7 * 2 * p["WROWS"]


def test_default_window_is_2pow22_rows():
    assert pk.proof_plan(G2, 16384, DEV)["log_bk"] == 22
    assert pk.proof_plan(G1, 150, DEV, force_stream=True)["log_bk"] == 16   # at least two windows per coset


def test_overrides_without_effect_below_their_heights():
    p = pk.proof_plan(G1, 128, DEV, force_stream=True, force_lowmem=True)   # 2^16 rows
    assert (p["stream"], p["lowmem"], p["log_s"]) == (0, 0, 0)
    p = pk.proof_plan(G1, 150, DEV, force_split=True)                       # 2^17 rows: the split level starts at 2^18
    assert (p["stream"], p["lowmem"], p["log_s"]) == (0, 0, 0)
    assert pk.proof_plan(G1, 150, DEV) == p


def test_window_override_is_clamped():
    for asked, got in ((3, 8), (8, 8), (17, 17), (30, 17), (0, 8)):
        assert pk.proof_plan(G1, 150, DEV, force_stream=True, stream_win_log=asked)["log_bk"] == got


def test_rejections_keep_code_and_text():
    with pytest.raises(RuntimeError, match=r"-5: supported trace heights: 2\^16 \.\. 2\^23 rows \(up to 16384 instances in one proof\)"):
        pk.proof_plan(G1, 16385, DEV)
    for field, value in (("rate_bits", 2), ("pow_bits", 0), ("num_queries", 257)):
        params = pk.default_params()
        setattr(params, field, value)
        with pytest.raises(RuntimeError, match=r"-5: unsupported StarkConfig \(only standard_fast_config shapes\)"):
            pk.proof_plan(FQ, 3, DEV, params=params)
    with pytest.raises(RuntimeError, match="-1"):
        pk.proof_plan(3, 1, DEV)
