"""Which GEMM kernels a call launches, pinned without a GPU: mmfd_debug_gemm_plan (a host-only export
of csrc/gemm.hip, not part of include/mmfd.h) must reproduce, for every case of
tests/golden/gemm_plans.json, what was recorded from the commit before the launch plan existed — the
launches (kernel instantiation, grid, block, dynamic LDS bytes), the split count, the row-sum mode, the
workspace layout, the three query values — and refuse what that commit refused, with the same message.
The Python side (kernels.g4_takes, kernels._probe_name) reads the plan and is pinned the same way.

A case is {"c": [dtype, c_dtype, trans_a, trans_b, M, N, K], "o": {options of gemm_args below},
"plan": [lines], "q": [workspace_bytes, splits, runs_split]}, with "rc" and "error" when the call is
refused ("plan" then holds nothing: a refused call is compared by code and message). "py" marks the
cases where that commit's Python functions were recorded: 1 when its _probe_name was asked alone,
[g4_takes] when both were; its _probe_name named the kernel it launched unless "probe_mirror_wrong"
holds the other name it gave, and "g4_takes_mirror_wrong" marks where it claimed the four-wave kernel
for a product that ran elsewhere (or the reverse) — the library's answer stands on both. "differs"
marks the cases that are meant to differ from that commit."""
import ctypes
import json
import os
import re

import pytest
import torch

from mmfd import kernels as K

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_plans.json")
BUILD = os.path.join(os.path.dirname(HERE), "multimodal-misinformation-detection_amd", "csrc", "build")
SWITCHES = ("MMFD_GEMM_V1", "MMFD_GEMM_F32_V1", "MMFD_GEMM_NARROW_G8", "MMFD_X6_SEGMENTED", "MMFD_G8_GROUP_M")
# dummy 16-B-aligned addresses, 4 GiB apart: a plan never dereferences them
PTR = {n: (i + 1) << 32 for i, n in enumerate(
    ("A", "B", "C", "bias", "residual", "aux", "seed", "workspace", "a_rowsum", "a_planes", "b_planes", "out_planes"))}
DT = {"f32": K.F32, "bf16": K.BF16}


def gemm_args(dtype, c_dtype, ta, tb, M, N, K_, *, act=0, bias=0, residual=0, res_first=0, aux=0, p=0.0, alpha=1.0,
              beta=0.0, splits=0, rowsum=0, rowsum_beta=0.0, a_planes=0, b_planes=0, a_only=0, b_only=0, out_planes=0,
              no_c=0, ws=0, pad=None, off=None, conv=None, null=(), struct_delta=0, **switches):
    """contiguous operands; `pad` adds to a leading dimension (lda, ldb, ldc, ldr, ldaux), `off` moves a
    pointer off its alignment, `null` zeroes pointers, `ws` is the workspace size in bytes (0: none),
    `conv` = [N, H, W, C, KH, KW, stride, pad, Ho, Wo]. The remaining options are library switches."""
    pad, off = pad or {}, off or {}
    a = K.GemmArgs()
    a.struct_size += struct_delta
    a.dtype, a.c_dtype = DT.get(dtype, 7), DT.get(c_dtype, 7)
    a.trans_a, a.trans_b, a.M, a.N, a.K = ta, tb, M, N, K_
    a.A, a.lda = PTR["A"] + off.get("A", 0), (M if ta else K_) + pad.get("lda", 0)
    a.B, a.ldb = PTR["B"] + off.get("B", 0), (N if tb else K_) + pad.get("ldb", 0)
    a.C, a.ldc = (0 if no_c else PTR["C"] + off.get("C", 0)), N + pad.get("ldc", 0)
    a.alpha, a.beta, a.splits = alpha, beta, splits
    a.ep.act, a.ep.residual_first, a.ep.salt = act, res_first, 7
    if bias:
        a.ep.bias = PTR["bias"] + off.get("bias", 0)
    if residual:
        a.ep.residual, a.ep.ldr = PTR["residual"] + off.get("residual", 0), N + pad.get("ldr", 0)
    if aux:
        a.ep.aux, a.ep.ldaux = PTR["aux"] + off.get("aux", 0), N + pad.get("ldaux", 0)
    if p > 0 or p < 0:
        a.ep.dropout_p, a.ep.seed = p, PTR["seed"]
    if rowsum:
        a.a_rowsum, a.a_rowsum_beta = PTR["a_rowsum"], rowsum_beta
    if a_planes:
        a.a_planes = PTR["a_planes"]
    if b_planes:
        a.b_planes = PTR["b_planes"]
    a.a_planes_only, a.b_planes_only = a_only, b_only
    if out_planes:
        a.ep.out_planes = PTR["out_planes"] + off.get("out_planes", 0)
    if ws:
        a.workspace, a.workspace_bytes = PTR["workspace"], ws
    geom = None
    if conv:
        geom = K.ConvGeomArgs(*conv)
        a.conv = ctypes.addressof(geom)
        a.lda = conv[3]
    for n in null:
        if n in ("seed", "aux"):
            setattr(a.ep, n, 0)
        else:
            setattr(a, n, 0)
    return a, geom


def switched(lib, o):
    """sets the library switches a case names and returns what undoes it"""
    old = [(lib.mmfd_debug_set_gemm_switch, n.encode(), lib.mmfd_debug_set_gemm_switch(n.encode(), o.get(n, 0)))
           for n in SWITCHES]
    mode = lib.mmfd_set_fp32_gemm_mode(0 if o.get("fp32") == "native" else 1)
    g4, kmax = K.set_g4_mode(o.get("g4", "gelu"), o.get("kmax", 1024))
    persist = K.set_g4_persist(o.get("persist", 1))

    def undo():
        for fn, n, v in old:
            fn(n, v)
        lib.mmfd_set_fp32_gemm_mode(mode)
        K.set_g4_mode(g4, kmax)
        K.set_g4_persist(persist)
    return undo


SWITCH_OPTS = SWITCHES + ("fp32", "g4", "kmax", "persist")


def py_tensors(case):
    """the CPU tensors of a case the Python functions are asked about (they read dtype, shape, stride
    and data_ptr only): 64-B aligned row-major views with the case's leading-dimension `pad` and
    pointer `off`"""
    dtype, c_dtype, ta, tb, M, N, K_ = case["c"]
    o = case["o"]
    td = {"f32": torch.float32, "bf16": torch.bfloat16}

    def mat(name, rows, cols, dt, ld=None):
        esz = 2 if dt == torch.bfloat16 else 4
        ld = cols + o.get("pad", {}).get(ld, 0)
        flat = torch.empty(rows * ld + 64, dtype=dt)
        start = (-flat.data_ptr() % 64) // esz + o.get("off", {}).get(name, 0) // esz
        return flat[start:start + rows * ld].view(rows, ld)[:, :cols]

    A = mat("A", *((K_, M) if ta else (M, K_)), td[dtype], "lda")
    B = mat("B", *((K_, N) if tb else (N, K_)), td[dtype], "ldb")
    out = mat("C", M, N, td[c_dtype], "ldc")
    opt = {n: mat(n, M, N, td[c_dtype], ld) if o.get(n) else None for n, ld in (("residual", "ldr"), ("aux", "ldaux"))}
    opt["bias"] = mat("bias", 1, N, torch.float32)[0] if o.get("bias") else None
    opt["a_rowsum"] = torch.empty(M) if o.get("rowsum") else None
    return A, B, out, opt


def py_answers(case):
    """(g4_takes, _probe_name) of kernels.py for a case"""
    _, _, ta, tb = case["c"][:4]
    o = case["o"]
    A, B, out, t = py_tensors(case)
    takes = None
    if not ta and not tb and not o.get("aux") and not o.get("rowsum"):
        takes = bool(K.g4_takes(A, B, o.get("act", 0), t["residual"], o.get("p", 0.0)))
    name = K._probe_name(A, B, out, ta, tb, t["residual"], o.get("act", 0), o.get("beta", 0.0), o.get("splits", 0),
                         alpha=o.get("alpha", 1.0), residual_first=bool(o.get("res_first", 0)),
                         dropout_p=o.get("p", 0.0), a_rowsum=t["a_rowsum"], aux=t["aux"], bias=t["bias"])
    return takes, name


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def plan():
    lib = K.load()
    fn = lib.mmfd_debug_gemm_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(K.GemmArgs), ctypes.c_char_p, ctypes.c_int64]
    lib.mmfd_debug_set_gemm_switch.restype = ctypes.c_int
    lib.mmfd_debug_set_gemm_switch.argtypes = [ctypes.c_char_p, ctypes.c_int]
    buf = ctypes.create_string_buffer(4096)

    def run(case):
        o = case["o"]
        a, _geom = gemm_args(*case["c"], **{k: v for k, v in o.items() if k not in SWITCH_OPTS})
        undo = switched(lib, o)
        try:
            rc = fn(ctypes.byref(a), buf, len(buf))
            err = lib.mmfd_last_error_string().decode() if rc else ""
            q = [lib.mmfd_gemm_workspace_bytes(ctypes.byref(a)), lib.mmfd_gemm_splits(ctypes.byref(a)),
                 lib.mmfd_gemm_runs_split(ctypes.byref(a))]
            py = py_answers(case) if "py" in case else None
        finally:
            undo()
        return rc, ([] if rc else buf.value.decode().splitlines()), err, q, py

    return run


def test_plans_match_the_recorded_launches(plan, golden):
    cases = golden["cases"]
    assert len(cases) >= 200
    bad = []
    for c in cases:
        rc, lines, err, q, _ = plan(c)
        if (rc, lines, err, q) != (c.get("rc", 0), c["plan"], c.get("error", ""), c["q"]):
            bad.append((c["c"], c["o"], (rc, lines, err, q), (c.get("rc", 0), c["plan"], c.get("error", ""), c["q"])))
    assert not bad, f"{len(bad)} of {len(cases)} plans differ; first: {bad[0]}"


def test_python_reads_the_plan(plan, golden):
    """g4_takes and _probe_name agree with the recorded commit wherever that commit's mirrors named
    the kernel it launched, and with the launch itself on the cases marked where they did not"""
    cases = [c for c in golden["cases"] if "py" in c]
    assert len(cases) >= 60 and sum(c["py"] != 1 for c in cases) >= 30
    bad = []
    for c in cases:
        takes, name = plan(c)[4]
        launched = next(l for l in c["plan"][1:] if not l.startswith("split3_kernel"))
        launched = re.split(r" (?:grid|tiles)=", launched)[0] + (" (split-K)" if " ws=0," in c["plan"][0] else "")
        assert c.get("probe_mirror_wrong") != launched, (c["c"], c["o"])
        want_takes = None if c["py"] == 1 else bool(c["py"][0])
        if c.get("g4_takes_mirror_wrong"):  # the recorded answer contradicts the recorded launch
            assert want_takes != c["plan"][0].startswith("path=g4 "), (c["c"], c["o"])
            want_takes = not want_takes
        if takes != want_takes or name != launched:
            bad.append((c["c"], c["o"], (takes, name), (want_takes, launched)))
    assert not bad, f"{len(bad)} of {len(cases)} differ; first: {bad[0]}"


def _demangled(sym):
    """a kernel's name as rocprof prints it, from its Itanium-mangled symbol: these kernels' template
    arguments are __bf16 (DF16b), float, int and bool literals only (binutils' c++filt does not know
    DF16b, so the few productions are read here)"""
    m = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", sym)
    at = m.end() + int(m.group(1))
    name, rest, args = sym[m.end():at], sym[at:], []
    if not rest.startswith("I"):
        return name
    rest = rest[1:]
    while not rest.startswith("E"):
        t = re.match(r"DF16b|f|Li(\d+)E|Lb([01])E", rest)
        assert t, sym
        args.append("__bf16" if t.group() == "DF16b" else "float" if t.group() == "f" else
                    t.group(1) if t.group(1) is not None else ("false", "true")[int(t.group(2))])
        rest = rest[t.end():]
    return f"{name}<{', '.join(args)}>"


def _kernel_symbols():
    """the kernels of the four GEMM objects, from the resource-usage remarks the Makefile keeps; None
    when the library was built elsewhere and came without its build directory"""
    names = set()
    if not os.path.exists(os.path.join(BUILD, "gemm.usage")):
        return None
    for unit in ("gemm", "gemm_f32out", "gemm_x6f", "gemm_g4"):
        mangled = re.findall(r"Function Name: (\S+)", open(os.path.join(BUILD, unit + ".usage")).read())
        assert mangled, unit
        names |= {_demangled(sym) for sym in mangled}
    return names


# kernels of these objects that no mmfd_gemm argument selects, with the reason
UNREACHED = {k: "launched inside mmfd_colsum, which picks the vector or scalar form from its own arguments' "
                "alignment; the plan names the mmfd_colsum follow-up and the workspace slice it gets"
             for k in ("colsum_partial_kernel<__bf16>", "colsum_partial_kernel<float>",
                       "colsum_partial_vec_kernel<__bf16>", "colsum_partial_vec_kernel<float>")}


def test_golden_covers_every_kernel_and_condition(golden):
    cases = golden["cases"]
    ok = [c for c in cases if c["plan"]]  # (a refused call and an empty one record no launch)
    lines = [l for c in ok for l in c["plan"][1:]]
    heads = [c["plan"][0] for c in ok]
    kernels = {re.split(r" (?:grid|tiles)=", l)[0] for l in lines if not l.startswith("mmfd_colsum")}
    # the kernel list: the build's own .usage files, which must name exactly the recorded commit's kernels;
    # a library that came without its build directory is measured against that recorded list alone
    built, want = _kernel_symbols(), set(golden["kernels"])
    assert len(want) == 68 + 24 + 13 + 7
    assert built is None or built == want, (sorted(built - want), sorted(want - built))
    assert kernels | set(UNREACHED) == want, (sorted(want - kernels), sorted(kernels - want))

    names = ("splits", "units", "rs_mode", "rs_nparts", "vec", "c_out", "planes", "ws_slabs", "ws_rowsum",
             "ws_a_planes", "ws_b_planes", "ws_total")

    def field(head, name):  # "path= splits= units= rs=,  flags=,,  ws=,,,,": the numbers in order
        return int(re.findall(r"-?\d+", head.split(" ", 1)[1])[names.index(name)])

    assert {h.split(" ")[0] for h in heads} == {"path=" + p for p in (
        "simple", "tile128", "tile128_conv", "tile256", "tile256_x6seg", "x6f", "x6f_conv", "g4")}
    assert {field(h, "rs_mode") for h in heads} == {0, 1, 2, 3}
    assert {f"splitk_reduce8_kernel<{t}, {p}>" for t in ("float", "__bf16") for p in (1, 2, 4, 8)} <= kernels
    assert {"splitk_reduce_kernel<float>", "splitk_reduce_kernel<__bf16>", "mmfd_reduce_partials_kernel"} <= kernels
    colsum = [c for c in ok if any(l.startswith("mmfd_colsum") for l in c["plan"])]
    assert {field(c["plan"][0], "ws_slabs") for c in colsum} == {-1, 0}
    assert {c["o"].get("act", 0) for c in ok} == set(range(9))
    assert {f"gemm_g4_kernel<{m}>" for m in range(7)} <= kernels
    assert {int(re.search(r"persist=(\d)", l).group(1)) for l in lines if l.startswith("gemm_g4")} == {0, 1}
    # ext_slab's three outcomes for GELU_D / MUL_AUX: the four-wave kernel, the split-operand ext kernel, a slab
    ext = [c for c in ok if c["o"].get("act") in (7, 8)]
    assert any("gemm_g4_kernel" in c["plan"][1] for c in ext)
    assert any("gemm256_x6f_ext_kernel" in " ".join(c["plan"]) for c in ext)
    assert any(field(c["plan"][0], "ws_slabs") == 0 and field(c["plan"][0], "splits") == 1 for c in ext)
    # planes handed over or split here, planes-only operands, out_planes with and without C
    x6 = [c for c in ok if c["q"][2]]
    assert {(bool(c["o"].get("a_planes")), bool(c["o"].get("b_planes"))) for c in x6} == {
        (False, False), (True, False), (False, True), (True, True)}
    assert any(c["o"].get("a_only") or c["o"].get("b_only") for c in ok)
    assert {field(h, "c_out") for h in heads if field(h, "planes")} == {0, 1}
    # every switch both ways, fp32 native and split
    for s in SWITCHES:
        assert {bool(c["o"].get(s)) for c in cases} == {False, True}, s
    assert {c["o"].get("fp32", "split") for c in cases} == {"native", "split"}
    # the workspace: absent, whole, slabs without planes (the fp32 MFMA fallback), fewer slabs than chosen
    assert any(c["q"][2] and c["o"].get("ws") and "path=tile256 " in c["plan"][0] and c["c"][0] == "f32" for c in ok)
    shrunk = [field(c["plan"][0], "splits") for c in ok if c["q"][1] > 1 and field(c["plan"][0], "splits") < c["q"][1]]
    assert 1 in shrunk and any(s > 1 for s in shrunk)
    # g4_epi: each condition that sends a bf16 -> bf16 forward product elsewhere, kmax on both sides. (Its
    # last checks — 16-B pointers, leading dims % 8 and >= the extent, tiles < 2^31 — cannot fail behind
    # mfma_ok and EpiArgs.vec, which ask the same of every product on the MFMA paths.)
    def g4(shape=(512, 768, 768), **o):
        hit = [c for c in ok if c["c"] == ["bf16", "bf16", 0, 0, *shape]
               and {k: v for k, v in c["o"].items() if k not in ("ws", "bias", "aux")} == o]
        assert hit, (shape, o)
        return hit[0]["plan"][0].startswith("path=g4 ")

    assert g4() and g4((32768, 768, 3072), kmax=4096) and not g4((512, 768, 2048), kmax=4096)  # (split-K there)
    for o in ({"g4": "off"}, {"g4": "on", "act": 1}, {"alpha": 0.5}, {"beta": 1.0}, {"splits": 2}, {"rowsum": 1},
              {"act": 2}, {"residual": 1, "res_first": 1}, {"pad": {"ldc": 4}}, {"kmax": 512}):
        assert not g4(**o), o
    for shape in ((520, 768, 768), (512, 776, 768), (512, 768, 800), (512, 768, 32), (512, 768, 2048)):
        assert not g4(shape), shape
    # x6_plan: each condition that keeps an fp32 product off split operands
    def runs_split(c, **o):
        hit = [x for x in cases if x["c"] == ["f32", "f32", *c] and all(x["o"].get(k) == v for k, v in o.items())]
        assert hit, (c, o)
        return hit[0]["q"][2]

    assert runs_split((0, 0, 512, 768, 768)) == 2 and runs_split((0, 0, 512, 768, 768), MMFD_X6_SEGMENTED=1) == 1
    assert runs_split((1, 0, 512, 768, 800)) == 2
    for c, o in (((0, 0, 512, 768, 768), {"fp32": "native"}), ((0, 0, 512, 768, 768), {"MMFD_GEMM_F32_V1": 1}),
                 ((0, 0, 512, 768, 772), {}), ((1, 0, 512, 768, 776), {}), ((0, 0, 98304, 768, 4096), {}),
                 ((0, 0, 4096, 128, 768), {})):
        assert runs_split(c, **o) == 0, (c, o)
    # shape edges
    assert {15, 16, 17, 4095, 4096} <= {c["c"][4] for c in ok} and {15, 16, 17, 64, 65, 128, 129} <= {c["c"][5] for c in ok}
    # every refusal of mmfd_gemm
    errors = " | ".join(c.get("error", "") for c in cases)
    for text in ("bad dtype", "bad c_dtype", "negative shape", "null C", "out_planes need", "ldc ", "bad act",
                 "backward act needs aux", "dropout needs seed", "dropout p must be < 1", "null operand",
                 "struct_size", "conv needs trans_a = 0", "conv needs trans_b = 0", "conv: bad geometry",
                 "conv: Ho / Wo", "conv: M != N*Ho*Wo", "conv: C must be a multiple", "conv: x must be 16-B aligned",
                 "conv: no a_rowsum", "conv: activation >= 2 GB", "conv with an unaligned", "only as split planes",
                 "with a_rowsum is not supported", "needs a workspace of", "conv on the segmented",
                 "a_rowsum without trans_a"):
        assert text in errors, text
    differs = [c for c in cases if c.get("differs")]
    assert len(differs) == 1 and "conv needs trans_b = 0" in differs[0]["error"]


def test_plan_export_needs_a_buffer(plan):
    lib = K.lib()
    a = K.GemmArgs()
    assert lib.mmfd_debug_gemm_plan(ctypes.byref(a), None, 0) == 1000
    assert "no buffer" in lib.mmfd_last_error_string().decode()


def test_group_m_switch_reaches_the_launcher_struct(plan):
    """MMFD_G8_GROUP_M changes no plan line (it is a launch argument of the 256x256 kernels), so the golden
    cases cannot show it: the setter's round trip does"""
    lib = K.lib()
    old = lib.mmfd_debug_set_gemm_switch(b"MMFD_G8_GROUP_M", 4)
    assert lib.mmfd_debug_set_gemm_switch(b"MMFD_G8_GROUP_M", 0) == 4  # (0 is raised to 1)
    assert lib.mmfd_debug_set_gemm_switch(b"MMFD_G8_GROUP_M", old) == 1


def test_unknown_switch_is_refused(plan):
    lib = K.lib()
    assert lib.mmfd_debug_set_gemm_switch(b"MMFD_NO_SUCH_SWITCH", 1) == -1
    assert "unknown switch" in lib.mmfd_last_error_string().decode()
