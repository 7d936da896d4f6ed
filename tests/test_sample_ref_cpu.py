"""The sampling rule without a GPU: tests/sample_ref.py (the float64 restatement the GPU tests hold csrc/sample.hip
to) against transformers' three warpers, the usability of the recorded seeds, the uniform draw, and the library's
host-side refusals (every one of them before a launch: no device is touched here)."""
import ctypes
import math

import numpy as np
import pytest

from tests import sample_ref as S

CASE_VOCABS = [7, 200, 1001, 30524]


@pytest.mark.parametrize("V", CASE_VOCABS)
def test_restatement_keeps_what_transformers_warpers_keep(V):
    pytest.importorskip("transformers")
    n = 0
    for si, (T, k, p) in enumerate(S.SETTINGS):
        for seed in S.case_seeds(V, si, 4):
            x = S.make_logits(V, seed)
            f = S.filter_ref(S.quotients(x, T), k, p)
            assert S.usable(f)
            hf = S.hf_kept(x, T, k, p)
            assert np.array_equal(hf, f.kept), (V, (T, k, p), seed, int(hf.sum()), f.n_kept)
            assert f.n_kept >= 1 and abs(f.probs.sum() - 1.0) < 1e-12
            n += 1
    assert n == 4 * len(S.SETTINGS)


@pytest.mark.parametrize("V", S.TEST_VOCABS)
def test_recorded_seeds_are_usable(V):
    for si, (T, k, p) in enumerate(S.SETTINGS):
        seeds = S.case_seeds(V, si)
        assert len(seeds) == S.MAX_ROWS and len(set(seeds)) == S.MAX_ROWS
        for seed in seeds:
            f = S.filter_ref(S.quotients(S.make_logits(V, seed), T), k, p)
            assert S.usable(f), (V, si, seed, f.gap)


def test_restatement_on_planted_rows():
    nan, inf = float("nan"), float("inf")
    # ties at the k-th value all survive top-k
    f = S.filter_ref(np.array([1, 3, 2, 2, 0, 2], np.float32), 2, 1.0)
    assert f.kept.tolist() == [False, True, True, True, False, True]
    # equal logits across the top-p boundary: the lower indices stay (masses 1/4 each, p = 0.6 keeps three)
    f = S.filter_ref(np.zeros(4, np.float32), 0, 0.6)
    assert f.kept.tolist() == [True, True, True, False]
    # top_p = 0 keeps the first entry of the order
    f = S.filter_ref(np.array([0, 2, 2, 1], np.float32), 0, 0.0)
    assert f.kept.tolist() == [False, True, False, False]
    # a NaN is never kept; -inf has no mass; a row without a number keeps nothing
    f = S.filter_ref(np.array([nan, -inf, 0.5, nan], np.float32), 0, 1.0)
    assert f.kept.tolist() == [False, False, True, False] and f.probs[2] == 1.0
    assert S.filter_ref(np.array([nan, -inf], np.float32), 1, 0.5).n_kept == 0
    # the draw: the lowest kept index whose inclusive prefix exceeds u
    f = S.filter_ref(np.log(np.array([0.25, 0.5, 0.25], np.float32)), 0, 1.0)
    assert [j for j in range(3) if S.accepted(f, j, 0.5)] == [1]
    assert S.accepted(f, 0, 0.25 - 1e-9) and S.accepted(f, 1, 0.25 + 1e-9) and not S.accepted(f, 2, 0.5)


def test_uniform_ref_grid_sensitivity_and_uniformity():
    base = S.uniform_ref(1234, 3, 5)
    assert 0.0 <= base < 1.0 and (base * 2 ** 24) == int(base * 2 ** 24)
    assert len({base, S.uniform_ref(1235, 3, 5), S.uniform_ref(1234, 4, 5), S.uniform_ref(1234, 3, 6)}) == 4
    bound = 1.63 / math.sqrt(4096)
    for seed in (0, 1, 1234, 2 ** 40 + 5):
        u = np.sort(np.array([S.uniform_ref(seed, t, r) for t in range(128) for r in range(32)]))
        assert ((0 <= u) & (u < 1)).all() and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
        n = u.size
        ks = max((np.arange(1, n + 1) / n - u).max(), (u - np.arange(n) / n).max())
        print(f"uniform_ref seed {seed}: KS distance {ks:.4f} (bound {bound:.4f})")
        assert ks < bound


def test_uniform_ref_is_the_librarys_hash():
    from mmfd import kernels as K
    K.load()
    for seed, step, row in ((0, 0, 0), (1234, 7, 31), (2 ** 40 + 5, 127, 2 ** 33 + 1)):
        assert S.uniform_ref(seed, step, row) == (K.dropout_hash(seed, step, row) >> 8) * 2.0 ** -24


def test_symbols_bound_and_workspace_query():
    from mmfd import kernels as K
    K.load()
    for name in ("mmfd_sample_select", "mmfd_sample_select_workspace_bytes", "mmfd_sample_select_resident_max"):
        assert name in K.SIGNATURES and hasattr(K.lib(), name)
    assert K.sample_select_resident_max() == S.RESIDENT_MAX
    for R, V in ((1, 1), (32, 30524), (5, S.RESIDENT_MAX + 1)):
        assert K.sample_select_workspace_bytes(R, V) >= 1
    for R, V in ((0, 10), (1, 0), (1, 2 ** 20 + 1)):
        with pytest.raises(RuntimeError, match="mmfd_sample_select_workspace_bytes"):
            K.sample_select_workspace_bytes(R, V)


def test_library_refuses_bad_arguments_before_any_launch():
    """the pointers are host buffers: a call that got past the checks would fault, a refused one never looks"""
    from mmfd import kernels as K
    K.load()
    lib = K.lib()
    V = 8
    logits = (ctypes.c_float * (2 * V))()
    ctl = (ctypes.c_int64 * 2)()
    out = (ctypes.c_int64 * 2)()
    probs = (ctypes.c_float * (2 * V))()
    ws = (ctypes.c_uint8 * 64)()
    P = lambda b: ctypes.cast(b, ctypes.c_void_p)  # noqa: E731
    good = dict(R=2, V=V, logits=P(logits), ldl=V, T=1.0, k=0, p=1.0, ctl=P(ctl), step=0, out=P(out), probs=None, ldp=0,
                kept=None, ws=P(ws), wsb=64)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mmfd_sample_select(a["R"], a["V"], a["logits"], a["ldl"], a["T"], a["k"], a["p"], a["ctl"], a["step"],
                                      a["out"], a["probs"], a["ldp"], a["kept"], a["ws"], a["wsb"], None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(R=0), dict(V=0), dict(ldl=V - 1), dict(probs=P(probs), ldp=V - 1), dict(T=0.0), dict(T=-1.0), dict(T=nan),
           dict(T=inf), dict(k=-1), dict(p=-0.1), dict(p=1.5), dict(p=nan), dict(step=-1), dict(logits=None),
           dict(ctl=None), dict(out=None), dict(ws=None), dict(wsb=K.sample_select_workspace_bytes(2, V) - 1)]
    for kw in bad:
        rc = call(**kw)
        msg = lib.mmfd_last_error_string().decode()
        assert rc == K.MMFD_ERR_INVALID and "mmfd_sample_select" in msg, (kw, rc, msg)


def test_python_argument_checks():
    from mmfd import kernels as K
    for bad in (dict(temperature=0.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1),
                dict(top_k=2.5), dict(top_p=1.1), dict(top_p=-0.1), dict(top_p=float("nan"))):
        with pytest.raises(ValueError):
            K.check_sampling(**dict(dict(temperature=1.0, top_k=0, top_p=1.0), **bad))
    assert K.check_sampling(0.7, 50, 0.9) == (0.7, 50, 0.9)
