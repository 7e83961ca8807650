"""The sparse-feature kernels (csrc/k9_sparse.hip) on the CPU: `sparse_ref` on a matrix small enough to read, the grid the case
table of tests/sparse_features_case.py has to cover, the rehearsal of every case with the fp32 CPU product standing in for the
device, and every refusal of pygat_project_sparse / pygat_wgrad_sparse.  The refusals come before any launch: no GPU is needed,
and a fake non-null address stands in for every device table (as in tests/test_abi.py)."""
import numpy as np
import pytest

import philox_ref as R
import sparse_features_case as case
from abi_support import P, lib  # noqa: F401

EINVAL = -1


# ---------------------------------------------------------------------------------------------------
# the ground truth and the case table
# ---------------------------------------------------------------------------------------------------
def test_sparse_ref_on_a_hand_worked_matrix(monkeypatch):
    """3 x 4, segments of 2 entries: column 0 is empty (one empty segment), column 1 has three entries (two segments),
    column 3 exactly two (one full segment)."""
    monkeypatch.setattr(case, "SEGMENT", 2)
    x = [[0, 5, 0, 7],
         [0, 6, 2, 0],
         [0, 9, 0, 8]]
    r = case.sparse_ref(x)
    want = dict(rowptr=[0, 2, 4, 6], col=[1, 3, 1, 2, 1, 3], val=[5, 7, 6, 2, 9, 8],
                trow=[0, 1, 2, 1, 0, 2], tval=[5, 6, 9, 2, 7, 8],
                colseg=[0, 1, 3, 4, 5], seg_col=[0, 1, 1, 2, 3], seg_begin=[0, 0, 2, 3, 4], seg_end=[0, 2, 3, 4, 6])
    assert r["nseg"] == 5
    for name in case.STRUCTURE_ARRAYS:
        assert r[name].tolist() == want[name], name
        assert r[name].dtype == (np.float32 if name in ("val", "tval") else np.int32), name


def test_sparse_ref_keeps_its_own_promises():
    """On both test matrices: segments tile every column's entries in order, none longer than 128, none across a column."""
    for kind in case.KINDS:
        x = case.matrix(kind, "norm").numpy()
        r = case.sparse_ref(x)
        assert r["rowptr"][-1] == len(r["col"]) == len(r["trow"]) == int((x != 0).sum())
        assert r["colseg"][-1] == r["nseg"] == len(r["seg_col"])
        assert r["nseg"] == case.FIN if kind == "rows" else r["nseg"] > case.FIN + 6      # columns of two and three segments
        at = 0
        for k in range(case.FIN):
            segs = range(r["colseg"][k], r["colseg"][k + 1])
            assert len(segs) == max(1, -(-int((x[:, k] != 0).sum()) // case.SEGMENT))
            for sg in segs:
                assert r["seg_col"][sg] == k and r["seg_begin"][sg] == at and 0 <= r["seg_end"][sg] - at <= case.SEGMENT
                at = r["seg_end"][sg]
            assert at == int((x[:, :k + 1] != 0).sum())
        assert np.array_equal(x[r["trow"], np.repeat(np.arange(case.FIN), np.bincount(r["col"], minlength=case.FIN))], r["tval"])


def test_matrices_hold_every_prescribed_length():
    pat, where = case.rows_matrix(case.N, case.FIN, 11)
    assert sorted(where) == sorted(set(case.ROW_COUNTS)) and [int(pat[i].sum()) for i in where.values()] == list(where)
    pat, where = case.cols_matrix(case.N, case.FIN, 12)
    assert sorted(where) == sorted(set(case.COL_COUNTS)) and [int(pat[:, k].sum()) for k in where.values()] == list(where)
    for kind in case.KINDS:
        for fl in case.FLAVOURS:
            x = case.matrix(kind, fl)
            assert 0.02 < float((x != 0).float().mean()) < 0.08
    assert set(case.matrix("rows", "exact").unique().tolist()) == {0.0, 1.0, 2.0, 3.0}


def test_the_case_table_covers_the_grid(lib):
    case.check_grid()
    for c in case.cases().values():
        assert c.Fp == lib.lib.pygat_padded_width(c.Fo)
    # the product's own wide masked shapes are in the table because the product reaches them
    assert lib.lib.pygat_headmask_supported(8, 16, 1) and lib.lib.pygat_headmask_supported(8, 32, 1)


def test_head_keep_is_the_generator_of_head_bits():
    keep = R.head_keep(case.SEED, case.STREAM, 5, 7, 13, 0.5)
    assert keep.shape == (13, 5, 7) and keep.dtype == bool
    bits = R.head_bits(case.SEED, case.STREAM, 5, 7, 8, 0.5)
    for h in range(8):
        assert np.array_equal((bits >> h) & 1, keep[h])
    assert np.array_equal(R.head_keep(case.SEED, case.STREAM, 5, 7, 32, 0.5)[:13], keep)     # head h does not depend on H


@pytest.mark.parametrize("name", case.case_names())
def test_case_passes_with_the_fp32_cpu_product(name):
    """The rehearsal of every GPU case: the fp32 CPU product under the case's masks passes the pricing; in the exact flavour
    it equals the fp64 product (the builder asserts every partial sum below 2^24 on the way)."""
    c = case.cases()[name]
    worst = c.rehearse()
    if c.flavour == "exact":
        assert max(worst.values()) == 0.0


# ---------------------------------------------------------------------------------------------------
# refusals, through the C ABI
# ---------------------------------------------------------------------------------------------------
def _project(L, **kw):
    a = dict(n=8, Fin=16, H=2, Fo=4, rowptr=P, col=P, val=P, Wcat=P, ldw=16, p=0.0, seed=None, stream_id=1, bits=None, Wh=P,
             Sk=None, s=None)
    assert kw and set(kw) <= set(a)          # (the defaults alone would be a valid call)
    a.update(kw)
    return L.lib.pygat_project_sparse(*a.values(), None)


def _wgrad(L, **kw):
    a = dict(n=8, Fin=16, H=2, Fo=4, nseg=16, colseg=P, seg_col=P, seg_begin=P, seg_end=P, row=P, val=P, p=0.0, seed=None,
             stream_id=1, bits=None, dWh=P, Gp=None, ldg=0, ws=P, dW=P, dWskip=None)
    assert kw and set(kw) <= set(a)
    a.update(kw)
    return L.lib.pygat_wgrad_sparse(*a.values(), None)


ENTRY = ((_project, "project_sparse"), (_wgrad, "wgrad_sparse"))


def _refused(L, fn, name, needle, **kw):
    rc = fn(L, **kw)
    msg = L.lib.pygat_last_error().decode()
    assert rc == EINVAL, (name, kw, rc, msg)
    assert msg.startswith(name + ":") and needle in msg, (name, kw, msg)


def test_both_entry_points_refuse_what_sp_setup_refuses(lib):
    for fn, name in ENTRY:
        skip = dict(Sk=P) if fn is _project else dict(Gp=P, dWskip=P, ldg=1024)
        _refused(lib, fn, name, "1024 output columns exceed 512", H=8, Fo=64, **skip)
        _refused(lib, fn, name, "dropout needs a seed or explicit mask bits", p=0.5)
        _refused(lib, fn, name, "explicit mask bits hold 8 heads", H=9, p=0.5, bits=P)
        _refused(lib, fn, name, "at most 32 heads", H=33, p=0.5, seed=P)
        for p in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
            _refused(lib, fn, name, "outside [0,1]", p=p, seed=P)
        _refused(lib, fn, name, "bad arguments", H=0)
        _refused(lib, fn, name, "bad arguments", Fo=257)          # no padded width
    _refused(lib, _project, "project_sparse", "520 output columns exceed 512", H=8, Fo=64, s=P)


def test_the_limits_themselves_pass_sp_setup(lib):
    """512 columns, 32 seeded heads, 8 heads of explicit bytes, p = 1 and p = 0 with a seed: each call gets as far as the next
    refusal (a short ldw / a null workspace), which names the sizes sp_setup let through."""
    for kw in (dict(H=8, Fo=64), dict(H=4, Fo=64, Sk=P), dict(H=32, Fo=16, p=0.5, seed=P), dict(H=8, Fo=32, Sk=P, p=0.5, bits=P),
               dict(H=32, Fo=4, p=1.0, seed=P), dict(H=8, Fo=8, p=0.0, seed=P, bits=P)):
        R_ = kw["H"] * case.padded_width(kw["Fo"])
        ncols = R_ * (2 if "Sk" in kw else 1)
        _refused(lib, _project, "project_sparse", f"bad arguments (ldw={ncols - 1}, {ncols} columns)", ldw=ncols - 1, **kw)
        w = {k: v for k, v in kw.items() if k != "Sk"}
        if "Sk" in kw:
            w.update(Gp=P, dWskip=P, ldg=R_)
        _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", ws=None, **w)


def test_project_sparse_refuses_its_own(lib):
    _refused(lib, _project, "project_sparse", "score columns are not formed under dropout", p=0.5, seed=P, s=P)
    _refused(lib, _project, "project_sparse", "score columns are not formed under dropout", p=0.5, bits=P, s=P)
    _refused(lib, _project, "project_sparse", "bad arguments (ldw=7, 8 columns)", ldw=7)
    _refused(lib, _project, "project_sparse", "bad arguments (ldw=9, 10 columns)", ldw=9, s=P)           # R + H
    _refused(lib, _project, "project_sparse", "bad arguments (ldw=17, 18 columns)", ldw=17, Sk=P, s=P)   # 2 R + H
    for arg in ("rowptr", "col", "val", "Wcat", "Wh"):
        _refused(lib, _project, "project_sparse", "bad arguments", **{arg: None})


def test_wgrad_sparse_refuses_its_own(lib):
    _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", nseg=15)                         # fewer segments than columns
    _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", Gp=P, dWskip=P, ldg=7)           # ldg < R
    _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", Gp=P, ldg=8)                     # Gp without dWskip
    for arg in ("colseg", "seg_col", "seg_begin", "seg_end", "row", "val", "dWh", "ws", "dW"):
        _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", **{arg: None})


def test_the_4_gib_guards_sit_exactly_at_the_bound(lib):
    """The kernels form byte offsets into Wcat, dWh and Gp in 32 bits: rows x row stride x 4 must stay below 2^32.  At the
    bound the call is refused; the largest size under it passes the guard and is refused by the NEXT check (nothing is
    launched either way)."""
    G = "4 GiB"
    # projection: Fin x ldw
    _refused(lib, _project, "project_sparse", G, Fin=1 << 20, ldw=1024)
    _refused(lib, _project, "project_sparse", G, Fin=(1 << 30) // 520 + 1, ldw=520, H=8, Fo=64)
    _refused(lib, _project, "project_sparse", "score columns", Fin=1 << 20, ldw=1023, p=0.5, seed=P, s=P)
    _refused(lib, _project, "project_sparse", "score columns", Fin=(1 << 30) // 520, ldw=520, H=8, Fo=32, p=0.5, seed=P, s=P)
    # weight gradient: n x R (dWh) ...
    wide = dict(H=8, Fo=32)                                                                  # R = 256
    _refused(lib, _wgrad, "wgrad_sparse", G, n=1 << 22, **wide)
    _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", n=(1 << 22) - 1, ws=None, **wide)
    # ... and n x ldg (Gp), with R far from its own bound
    _refused(lib, _wgrad, "wgrad_sparse", G, n=1 << 20, Gp=P, dWskip=P, ldg=1024)
    _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", n=1 << 20, Gp=P, dWskip=P, ldg=1023, ws=None)
    _refused(lib, _wgrad, "wgrad_sparse", G, n=(1 << 22) - 1, Gp=P, dWskip=P, ldg=257, **wide)
    _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", n=(1 << 22) - 1, Gp=P, dWskip=P, ldg=256, ws=None, **wide)
    # ldg does not count without Gp
    _refused(lib, _wgrad, "wgrad_sparse", "bad arguments", n=1 << 20, ldg=1 << 40, ws=None)
