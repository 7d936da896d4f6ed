"""The launch trace of BLIP captioning: every call that mmfd.blip and mmfd.blocks make into mmfd.kernels during the
first `generate(use_graph=True)` of a fresh model (and during one `forward_logits`), against
tests/golden/blip_decode_trace.json. The id tests do not see a launch that leaves the ids alone (the LM head of a
forced greedy step is one); this file pins what a captured captioning graph holds, and so what it costs.

A trace is a list of strings, one per call: the function's name and its arguments in order, tensors as dtype, shape
and strides, lists element-wise, numbers / bools / None / strings as values; never an address. `_capture` runs the
loop twice, as warm-up on a side stream and under capture, with no host read in between; each call is filed by
whether its stream was capturing. What is not captured is the driver's host-side prelude (argument checks, workspace
sizes, pointer tables: no launch, compared as a sorted list) and, from the vision tower's `patchify` on, the warm-up.
The warm-up differs from the captured half only in the `cast` calls with which it builds the weight shadows and
packed weights (the capture finds them built): that is asserted, and both halves are compared with the golden.

The golden was recorded with this module on an MI355X from the package as it stood before the three decoding loops
became one:  python -m tests.test_blip_decode_trace_gpu OUT.json  (it uses `generate` and `forward_logits` only).
Distinct call strings are stored once, traces as lists of indices."""
import functools
import inspect
import json
import os
import sys

import pytest
import torch

from tests import blip_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(R.G, "blip_decode_trace.json")
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2, suppress_tokens=[14, 87])
SAMPLE = dict(do_sample=True, num_return_sequences=2, top_k=20, top_p=0.9, seed=5)
BEAMS = dict(num_beams=3, early_stopping=True)
# name -> (rows, prompted, generate's extra arguments); "forward" is forward_logits
CASES = {
    "greedy": (4, True, {}),
    "greedy_proc": (4, True, PROC),
    "sample": (4, True, SAMPLE),
    "sample_proc": (4, True, {**SAMPLE, **PROC}),
    "beams": (4, True, BEAMS),
    "beams_proc": (4, True, {**BEAMS, **PROC}),
    "greedy_wide": (40, False, {}),
    "forward": (4, False, None),
}
PRECISIONS = ("fp32", "bf16")


def _fmt(a):
    if isinstance(a, torch.Tensor):
        return f"{str(a.dtype)[6:]}{list(a.shape)}/{list(a.stride())}"
    if isinstance(a, (list, tuple)):
        return "[" + ", ".join(_fmt(x) for x in a) + "]"
    if isinstance(a, dict):
        return "{" + ", ".join(f"{k}: {_fmt(v)}" for k, v in a.items()) + "}"
    if a is None or isinstance(a, (bool, int, float, str)):
        return repr(a)
    if isinstance(a, torch.dtype):
        return str(a)[6:]
    return f"<{type(a).__name__}>"


def wrap_kernels(setattr_, warm, graph):
    """replace every public function defined in mmfd.kernels by a wrapper that files the call's string in `graph`
    when its stream is capturing, else in `warm`. setattr_(module, name, value): monkeypatch.setattr in the tests"""
    from mmfd import kernels as K

    def wrapper(name, fn):
        @functools.wraps(fn)
        def call(*args, **kw):
            s = ", ".join([_fmt(a) for a in args] + [f"{k}={_fmt(v)}" for k, v in kw.items()])
            (graph if torch.cuda.is_current_stream_capturing() else warm).append(f"{name}({s})")
            return fn(*args, **kw)
        return call

    for name, fn in list(vars(K).items()):
        if name.startswith("_") or name in ("lib", "load"):
            continue
        if inspect.isfunction(fn) and fn.__module__ == K.__name__:
            setattr_(K, name, wrapper(name, fn))


def inputs():
    z, cfg, W = R.load_fixture()
    px4 = torch.from_numpy(z["pixel_values"])
    noise = torch.randn(36, 3, 80, 80, generator=torch.Generator().manual_seed(40))  # as tests/test_caption_wide_gpu.py
    px40 = torch.cat([px4, (noise * 64).round().clamp(-255, 255) / 64])
    return dict(cfg=cfg, W=W, px={4: px4, 40: px40}, prompt=torch.tensor([cfg["text"]["bos_token_id"], 7, 11]))


def run_case(fx, case, precision):
    """runs `case` on a fresh model; the kernels must be wrapped already"""
    rows, prompted, extra = CASES[case]
    m = R.load_model(fx["cfg"], fx["W"], precision, DEV)
    if extra is None:
        m.forward_logits(fx["px"][rows], torch.full((rows, 4), 4, dtype=torch.int64))  # forced ids [4, 4], every id 4
    else:
        m.generate(fx["px"][rows], fx["prompt"] if prompted else None, max_new_tokens=3, use_graph=True, **extra)
    torch.cuda.synchronize()


def _without_casts(trace):
    return [c for c in trace if not c.startswith("cast(")]


def _split(trace):
    """(the host-side prelude, sorted; the loop): the loop starts at the vision tower's first call"""
    i = next(i for i, c in enumerate(trace) if c.startswith("patchify("))
    return sorted(trace[:i]), trace[i:]


@pytest.fixture(scope="module")
def fx():
    return inputs()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {k: {h: [g["calls"][i] for i in idx] for h, idx in t.items()} for k, t in g["traces"].items()}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_launch_trace_is_the_recorded_one(fx, golden, monkeypatch, case, precision):
    warm, graph = [], []
    wrap_kernels(monkeypatch.setattr, warm, graph)
    run_case(fx, case, precision)
    want = golden[f"{case}-{precision}"]
    print(f"{case}-{precision}: {len(warm)} calls outside a capture, {len(graph)} captured; "
          f"recorded {len(want['warm'])}, {len(want['graph'])}")
    prelude, loop = _split(warm)
    if CASES[case][2] is None:
        assert not graph and loop  # forward_logits captures nothing
    else:
        assert graph and _without_casts(loop) == graph
    assert graph == want["graph"]
    assert (prelude, loop) == _split(want["warm"])


def record(path):
    from mmfd import kernels as K
    fx = inputs()
    calls, traces = {}, {}
    saved = {}

    def set_(mod, name, value):
        saved.setdefault(name, getattr(mod, name))
        setattr(mod, name, value)

    for case in CASES:
        for precision in PRECISIONS:
            warm, graph = [], []
            wrap_kernels(set_, warm, graph)
            try:
                run_case(fx, case, precision)
            finally:
                for name, fn in saved.items():
                    setattr(K, name, fn)
                saved.clear()
            traces[f"{case}-{precision}"] = {h: [calls.setdefault(c, len(calls)) for c in t]
                                             for h, t in (("warm", warm), ("graph", graph))}
            print(f"{case}-{precision}: {len(warm)} + {len(graph)} calls, without casts "
                  f"{'equal' if not graph or _without_casts(_split(warm)[1]) == graph else 'DIFFERENT'}", flush=True)
    with open(path, "w") as f:
        json.dump({"calls": list(calls), "traces": traces}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(calls)} distinct calls -> {path}")


if __name__ == "__main__":
    record(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
