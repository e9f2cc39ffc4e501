"""The root-link check on the GPU (csrc/root_links.hip, bn254s_root_links_check_batch) against tools/root_links_ref.py, row for
row, codes and bases: for every front-end the crafted rows of the reference - every code, the edge inputs x = 0 with both signs,
Fq2 elements with c0 = 0 or c1 = 0 and roots (0, t), y = 1 and y = p - 1, u = 0 and u = +-1/2, four u of every branch of the map -
mixed into honest rows that the front-end itself made on the device, at one lane, one short of a block of 64, one block, one over
and a ragged tail past two blocks; all of them in one call, in both orders, with and without the caller's jobs; and the range
check of the host with a context to hold its text."""
import ctypes as C

import numpy as np
import pytest

from tools import root_links_ref as rl
from tools import synth

P = synth.P
SIZES = [1, 63, 64, 65, 130]
NAMES = ("g1_recover", "g2_recover", "fq_sqrt", "fq2_sqrt", "map_to_g1")


@pytest.fixture(scope="module")
def crafted():
    return {what: rl.cases(what) for what in rl.WHATS}


@pytest.fixture(scope="module")
def honest(gpu_ctx):
    """what -> Rows of 130 uniform inputs as the front-end of `what` returns them: one *_batch call per kind, read-only."""
    out = {}
    for what in rl.WHATS:
        xs, sgns = rl.random_inputs(what, 130, seed=0x686F6E)
        rows, _ = rl.device_rows(gpu_ctx, what, rl.to_words(what, xs), sgns)
        for a in rows:
            a.setflags(write=False)
        out[what] = rows
    return out


def _take(what, rows, idx):
    """The rows idx of a call as a call."""
    J = rl.JOBS[what]
    idx = np.asarray(idx)
    jdx = (J * idx[:, None] + np.arange(J)[None, :]).reshape(-1)
    return rl.Rows(*(np.ascontiguousarray(a[jdx] if k in (3, 5) else a[idx]) for k, a in enumerate(rows)))


def _mixed(what, honest_rows, crafted_rows, n):
    """n rows: crafted ones at the even places, at both ends of the first wave and past the block boundary, honest ones
    between them; which crafted ones depends on n, so that the five sizes walk through them."""
    k = len(crafted_rows.xs)
    parts, which = [], []
    for i in range(n):
        if i % 2 == 0 or i in (63, 65, n - 1):
            parts.append(_take(what, crafted_rows, [(i + n) % k]))
            which.append((i + n) % k)
        else:
            parts.append(_take(what, honest_rows, [i]))
            which.append(None)
    return rl.Rows(*(np.concatenate(c) for c in zip(*parts))), which


def _check(ctx, what, rows, jobs=True):
    return ctx.root_links_check_batch(what, rows.xs, rows.out, rows.flags, sgns=rows.sgns, root_ok=rows.root_ok,
                                      fq_jobs=rows.jobs if jobs else None)


def _same(got, want, label):
    bad = np.nonzero(got != want)[0]
    assert not bad.size, (label, [(int(j), int(got[j]), int(want[j])) for j in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("what", rl.WHATS)
def test_sizes(gpu_ctx, honest, crafted, what, n):
    rows, which = _mixed(what, honest[what], crafted[what][0], n)
    want, want_bases = rl.codes(what, rows)
    codes, bases = _check(gpu_ctx, what, rows)
    assert codes.shape == (n,) and codes.dtype == np.uint8 and bases.shape == (rl.JOBS[what] * n, 4)
    _same(codes, want, NAMES[what])
    assert np.array_equal(bases, want_bases)
    for i, j in enumerate(which):  # the crafted rows have the code they were made for, the honest rows none
        assert codes[i] == (0 if j is None else crafted[what][1][j]), (i, j)
    if n == 130:  # once: without the caller's jobs the job codes give way to what follows them, and the bases are the same
        codes2, bases2 = _check(gpu_ctx, what, rows, jobs=False)
        _same(codes2, rl.codes(what, rows, with_jobs=False)[0], NAMES[what])
        assert np.array_equal(bases2, want_bases) and not ((codes2 == 1) | (codes2 == 2)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("what", rl.WHATS)
def test_honest_rows_and_every_crafted_row(gpu_ctx, honest, crafted, what):
    h = honest[what]
    codes, bases = _check(gpu_ctx, what, h)
    assert not codes.any() and np.array_equal(bases, h.jobs[:, 4:])  # the front-end's own jobs hold the bases
    assert len(set(int(f) for f in h.flags)) == 2  # both flag values are among them
    rows, want, names = crafted[what]
    k = len(want)
    codes, bases = _check(gpu_ctx, what, rows)
    assert [(names[i], int(codes[i])) for i in range(k) if codes[i] != want[i]] == []
    assert np.array_equal(bases, rl.codes(what, rows)[1])
    # the other way round: a code depends on its row alone
    back = _take(what, rows, np.arange(k)[::-1])
    codes, _ = _check(gpu_ctx, what, back)
    assert np.array_equal(codes, want[::-1])
    # sgns NULL is all zero
    if what in (rl.G2_RECOVER, rl.FQ_SQRT, rl.FQ2_SQRT):
        zeros = rows._replace(sgns=np.zeros(k, np.uint8))
        got, _ = gpu_ctx.root_links_check_batch(what, rows.xs, rows.out, rows.flags, sgns=None, root_ok=rows.root_ok, fq_jobs=rows.jobs)
        assert np.array_equal(got, rl.codes(what, zeros)[0])


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.gpu
@pytest.mark.parametrize("what", rl.WHATS)
def test_a_coordinate_not_below_p_is_named(gpu_ctx, honest, what):
    lib, h = gpu_ctx._lib, gpu_ctx._h
    rows = _take(what, honest[what], np.arange(70))
    J, iw, ow = rl.JOBS[what], rl.IN_WORDS[what], rl.OUT_WORDS[what]
    raw, raw_bases = np.full(73, 9, np.uint8), np.full((J * 70 + 1, 4), 9, np.uint64)

    def call(r, what_=what, n=70):
        return lib.bn254s_root_links_check_batch(h, what_, _vp(r.xs), _vp(r.sgns), n, _vp(r.out), _vp(r.flags), _vp(r.root_ok), _vp(r.jobs),
                                                 _vp(raw), _vp(raw_bases))

    text = lambda: lib.bn254s_last_error(h).decode()
    in_name = "u" if what == rl.MAP_TO_G1 else "x"
    out_name = "roots" if what in (rl.FQ_SQRT, rl.FQ2_SQRT) else "points"
    at = 0 if what in (rl.FQ_SQRT, rl.FQ2_SQRT) else iw  # where the y / root begins
    claimed = rows.root_ok if what in (rl.FQ_SQRT, rl.FQ2_SQRT) else np.ones(70, np.uint8) if what == rl.MAP_TO_G1 else rows.flags
    yes, no = [i for i in range(70) if claimed[i]], [i for i in range(70) if not claimed[i]]
    for v in (P, P + 1):
        xs = rows.xs.copy()
        xs[66, iw - 4:] = synth._to_words(v)
        xs[68, :4] = synth._to_words(v)  # the first such row is the one named
        assert call(rows._replace(xs=xs)) == -1
        assert text() == f"root_links_check: {in_name}_66 " + ("has c1 not below p" if iw == 8 else "is not below p")
        out = rows.out.copy()
        out[yes[-1], ow - 4:] = synth._to_words(v)
        coord = {rl.G1_RECOVER: "has y", rl.G2_RECOVER: "has y.c1", rl.FQ_SQRT: "is", rl.FQ2_SQRT: "has c1", rl.MAP_TO_G1: "has y"}[what]
        assert call(rows._replace(out=out)) == -1
        assert text() == f"root_links_check: {out_name}_{yes[-1]} {coord} not below p"
        assert call(rows._replace(xs=xs, out=out)) == -1 and text().startswith(f"root_links_check: {in_name}_66 ")  # the inputs first
    assert call(rows, what_=5) == -1 and call(rows, n=0) == -1  # (no text: the shape answers first)
    assert (raw == 9).all() and (raw_bases == 9).all()
    # rows that are never read as a field element are not range-checked: the x of a point is compared (code 4), the y of a
    # clear flag / the root of a clear root_ok is compared with zero (code 5)
    out = rows.out.copy()
    expect = np.zeros(70, np.uint8)
    if at:
        out[yes[0], :4] = synth._to_words(P)
        expect[yes[0]] = rl.CARRY
    if no:
        out[no[0], at:at + 4] = synth._to_words(P + 1)
        expect[no[0]] = rl.NOT_ZERO
    assert call(rows._replace(out=out)) == 0
    assert np.array_equal(raw[:70], expect) and (raw[70:] == 9).all()  # every lane writes its own byte and no other
    assert np.array_equal(raw_bases[:J * 70], rows.jobs[:, 4:]) and (raw_bases[J * 70:] == 9).all()
