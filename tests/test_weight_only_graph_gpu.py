"""HIP-graph replay of weights-only evaluations (engine.WEIGHT_ONLY_GRAPH) on the GPU: a replay returns the bytes of the eager
walk for inputs other than the captured ones, the knob tuple selects the graph, foreign hooks / autocast / a refused layer keep
the model eager, and — in a fresh child process — the graph set survives switches between the integer and the weights-only
state and invalidate_plans() (the pool handle is dropped with the last graph)."""
import os
import subprocess
import sys

import pytest
import torch

from golden_util import fixture_inputs, load_fixture
from test_weight_only_gpu import BOUNDS, _metrics, _resume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cifar_tiny", "ldm_tiny", "sd_tiny", "ldm_updown_tiny"]
KNOBS = ("WEIGHT_ONLY_KERNEL", "WEIGHT_ONLY_ATTN", "WEIGHT_ONLY_FUSE", "WEIGHT_ONLY_FUSE_WIDE", "WEIGHT_ONLY_FUSE_MOD",
         "WEIGHT_ONLY_FUSE_DDIM", "WEIGHT_ONLY_SPLITK", "WEIGHT_ONLY_TEMB", "WEIGHT_ONLY_GRAPH")


@pytest.fixture
def knobs():
    from qdiff import engine
    prev = {n: getattr(engine, n) for n in KNOBS}
    fused = dict(engine.WONLY_FUSED)
    yield engine
    for n, v in prev.items():
        setattr(engine, n, v)
    engine.WONLY_FUSED.clear()                         # (the fused routes add their keys on first use: other tests compare the dict)
    engine.WONLY_FUSED.update(fused)


def all_knobs(engine, on, dt=torch.float16):
    """The layer knob, and with on=True every other weights-only knob except replay itself."""
    engine.set_weight_only_kernel(dt)
    engine.set_weight_only_attention(dt if on else None)
    for f in (engine.set_weight_only_fusion, engine.set_weight_only_fusion_wide, engine.set_weight_only_fusion_mod,
              engine.set_weight_only_fusion_ddim, engine.set_weight_only_splitk, engine.set_weight_only_temb):
        f(on)


def inputs(fx, dev):
    """The fixture's test inputs and a second set of the same shapes."""
    x, t, c = (a.to(dev) if a is not None else None for a in fixture_inputs(fx, "test"))
    g = torch.Generator(device=dev).manual_seed(5)
    x2 = torch.randn(x.shape, device=dev, generator=g)
    t2 = (t + 37) % 1000
    c2 = torch.randn(c.shape, device=dev, generator=g) if c is not None else None
    return (x, t, c), (x2, t2, c2)


def run(qnn, a):
    x, t, c = a
    return (qnn(x, t, c) if c is not None else qnn(x, t)).clone()


def _model(name, dev):
    fx = load_fixture(f"model_{name}.pt")
    qnn = _resume(fx, dev)
    qnn.set_quant_state(True, False)
    return fx, qnn


@pytest.mark.parametrize("name", NAMES)
def test_replay_equals_eager_with_every_knob_on(cuda, knobs, name):
    fx, qnn = _model(name, cuda)
    all_knobs(knobs, True)
    a1, a2 = inputs(fx, cuda)
    with torch.no_grad():
        e1, e2 = run(qnn, a1), run(qnn, a2)
        assert not qnn._graphs                                         # knob off: nothing was captured
        knobs.set_weight_only_graph(True)
        qnn.enable_hip_graphs(True)
        assert qnn._wonly_token() >= 0
        n0 = knobs.WONLY_TEMB[0]
        g1 = run(qnn, a1)            # captures
        n1 = knobs.WONLY_TEMB[0]
        g2 = run(qnn, a2)            # replays with new inputs
        g1b = run(qnn, a1)
        assert len(qnn._graphs) == 1 and knobs.WONLY_TEMB[0] == n1 > n0          # a replay runs no Python
        qnn.enable_hip_graphs(False)
    torch.cuda.synchronize()
    assert torch.equal(e1, g1) and torch.equal(e2, g2) and torch.equal(g1, g1b)
    assert qnn.__dict__.get("_graph_pool") is None


@pytest.mark.parametrize("name", NAMES)
def test_replay_with_the_layer_knob_alone(cuda, knobs, name):
    """Only QDIFF_WEIGHT_ONLY=fp16: the library's attention and norms are inside the capture."""
    fx, qnn = _model(name, cuda)
    all_knobs(knobs, False)
    a1, a2 = inputs(fx, cuda)
    with torch.no_grad():
        e1, e2 = run(qnn, a1), run(qnn, a2)
        knobs.set_weight_only_graph(True)
        qnn.enable_hip_graphs(True)
        g1, g2, g1b = run(qnn, a1), run(qnn, a2), run(qnn, a1)
        assert len(qnn._graphs) == 1
        qnn.enable_hip_graphs(False)
    torch.cuda.synchronize()
    d, cos = _metrics(g1, fx["out_w"])
    print(f"\n[{name}] layer knob alone, replayed: {d:.3e} of range, cosine {cos:.7f}; "
          f"replay == eager: {torch.equal(e1, g1)}, {torch.equal(e2, g2)}, {torch.equal(g1, g1b)}")
    assert torch.equal(e1, g1) and torch.equal(e2, g2) and torch.equal(g1, g1b)


def test_knob_off_never_captures(cuda, knobs):
    fx, qnn = _model("ldm_tiny", cuda)
    all_knobs(knobs, True)
    knobs.set_weight_only_graph(False)
    a1, _ = inputs(fx, cuda)
    with torch.no_grad():
        ys = [run(qnn, a1) for _ in range(3)]
        qnn.enable_hip_graphs(True)
        ys += [run(qnn, a1) for _ in range(2)]
    assert qnn._graphs == {} and qnn._wonly_token() == -1 and all(torch.equal(y, ys[0]) for y in ys)


def test_default_replay_captures_on_second_sight(cuda, knobs):
    """Without enable_hip_graphs(): the rules of the integer state — the second evaluation of a signature captures."""
    fx, qnn = _model("ldm_tiny", cuda)
    all_knobs(knobs, True)
    knobs.set_weight_only_graph(True)
    a1, _ = inputs(fx, cuda)
    assert qnn._graphs == {} and qnn._graph_after == 1                # the defaults of the constructor
    with torch.no_grad():
        y1 = run(qnn, a1)
        assert len(qnn._graphs) == 0
        y2 = run(qnn, a1)
        assert len(qnn._graphs) == 1
        y3 = run(qnn, a1)
    assert torch.equal(y1, y2) and torch.equal(y1, y3)


def test_two_knob_tuples_are_two_graphs(cuda, knobs):
    fx, qnn = _model("sd_tiny", cuda)
    all_knobs(knobs, True)
    a1, a2 = inputs(fx, cuda)
    with torch.no_grad():
        knobs.set_weight_only_attention(None)
        e_off = run(qnn, a1)
        knobs.set_weight_only_attention(torch.float16)
        e_on = run(qnn, a1)
        knobs.set_weight_only_graph(True)
        qnn.enable_hip_graphs(True)
        tok = qnn._wonly_token()
        for i in range(3):
            knobs.set_weight_only_attention(None)
            assert torch.equal(run(qnn, a1), e_off)
            knobs.set_weight_only_attention(torch.float16)
            assert torch.equal(run(qnn, a1), e_on)
            assert len(qnn._graphs) == 2 and qnn._wonly_token() == tok
        qnn.enable_hip_graphs(False)
    assert not torch.equal(e_off, e_on)


def test_hooks_registered_after_capture_keep_the_model_eager(cuda, knobs):
    from qdiff.quant_block import QuantBasicTransformerBlock
    fx, qnn = _model("sd_tiny", cuda)
    all_knobs(knobs, True)
    knobs.set_weight_only_graph(True)
    a1, _ = inputs(fx, cuda)
    with torch.no_grad():
        qnn.enable_hip_graphs(True)
        ys = [run(qnn, a1) for _ in range(3)]
        assert len(qnn._graphs) == 1
        g = next(iter(qnn._graphs.values()))
        replays = []
        orig = g.graph.replay
        g.graph.replay = lambda: (replays.append(1), orig())[1]
        fired = []
        mod = next(m for m in qnn.modules() if isinstance(m, QuantBasicTransformerBlock))
        h = mod.register_forward_hook(lambda _m, _a, _o: fired.append(1))
        y_hooked = run(qnn, a1)
        assert fired and not replays and len(qnn._graphs) == 1
        # (a hooked block keeps the composition its hook expects, so the eager walk it falls back to is the HOOKED model's: the
        # bytes to compare with are those of the same model with replay switched off)
        knobs.set_weight_only_graph(False)
        y_hooked_eager = run(qnn, a1)
        knobs.set_weight_only_graph(True)
        assert len(fired) == 2 and not replays and len(qnn._graphs) == 1
        h.remove()
        y_back = run(qnn, a1)
        assert replays and len(fired) == 2
        qnn.enable_hip_graphs(False)
    torch.cuda.synchronize()
    assert all(torch.equal(y, ys[0]) for y in ys[1:] + [y_back])
    assert torch.equal(y_hooked, y_hooked_eager)
    d, cos = _metrics(y_hooked, fx["out_w"])
    assert d <= BOUNDS[torch.float16][0] and cos >= BOUNDS[torch.float16][1]


def test_autocast_captures_nothing(cuda, knobs):
    fx, qnn = _model("ldm_tiny", cuda)
    all_knobs(knobs, True)
    knobs.set_weight_only_graph(True)
    a1, _ = inputs(fx, cuda)
    with torch.no_grad():
        qnn.enable_hip_graphs(True)
        with torch.autocast("cuda"):
            y = [run(qnn, a1) for _ in range(3)]
        assert qnn._graphs == {}
        qnn.enable_hip_graphs(False)
    d, cos = _metrics(y[0], fx["out_w"])
    tol, cmin = BOUNDS["autocast"]
    assert d <= tol and cos >= cmin


def test_refused_layer_captures_nothing(cuda, knobs):
    import qdiff
    from qdiff.quant_layer import UniformAffineQuantizer
    fx, qnn = _model("ldm_tiny", cuda)
    all_knobs(knobs, True)
    knobs.set_weight_only_graph(True)
    a1, _ = inputs(fx, cuda)
    m = [m for m in qnn.modules() if isinstance(m, qdiff.QuantModule)][3]
    m.weight_quantizer = UniformAffineQuantizer(n_bits=4, channel_wise=False, scale_method="max").to(cuda)
    with torch.no_grad():
        qnn.enable_hip_graphs(True)
        ys = [run(qnn, a1) for _ in range(3)]
        assert qnn._wonly_token() == -1 and qnn._graphs == {}
        qnn.enable_hip_graphs(False)
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


CHILD = r"""
import sys, torch
sys.path[:0] = [{tests!r}, {pkg!r}, {root!r}]
from golden_util import fixture_inputs, load_fixture
from test_weight_only_gpu import _resume
from test_weight_only_graph_gpu import all_knobs, inputs, run
from qdiff import engine
dev = torch.device("cuda:0")
fx = load_fixture("model_sd_tiny.pt")
qnn = _resume(fx, dev)
all_knobs(engine, True)
a1, a2 = inputs(fx, dev)
with torch.no_grad():
    qnn.enable_hip_graphs(False)
    qnn.set_quant_state(True, False)
    w1, w2 = run(qnn, a1), run(qnn, a2)
    qnn.set_quant_state(True, True)
    i1, i2 = run(qnn, a1), run(qnn, a2)
    engine.set_weight_only_graph(True)
    qnn.enable_hip_graphs(True)
    steps = []
    def check(tag, e1, e2, kept=1):
        g1, g2, g1b = run(qnn, a1), run(qnn, a2), run(qnn, a1)
        ok = torch.equal(g1, e1) and torch.equal(g2, e2) and torch.equal(g1b, e1) and len(qnn._graphs) == kept
        print(tag, ok, len(qnn._graphs), flush=True)
        steps.append(ok)
    qnn.set_quant_state(True, False)
    check("weights-only", w1, w2)
    qnn.set_quant_state(True, True)
    check("integer", i1, i2, kept=2)          # (the integer key holds the slot of the prepared context: one graph per context)
    qnn.set_quant_state(True, False)
    check("weights-only again", w1, w2)
    qnn.invalidate_plans()
    assert qnn.__dict__.get("_graph_pool") is None and not qnn._graphs
    check("after invalidate_plans", w1, w2)
torch.cuda.synchronize()
sys.exit(0 if all(steps) and len(steps) == 4 else 3)
"""


def test_state_switches_recapture_in_a_fresh_process(cuda):
    """capture weights-only -> (True, True) and capture -> back and capture -> invalidate_plans() and capture, every output equal
    to its eager counterpart.  Each switch empties the graph set, so each capture must open a pool of its own."""
    code = CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=os.path.join(ROOT, "q-diffusion_amd"), root=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=240)
    print(r.stdout[-2000:], r.stderr[-2000:])
    if r.returncode not in (0, 3):                         # the child died (abort, fault): nothing else is started on this GPU
        pytest.exit(f"the child of test_state_switches_recapture_in_a_fresh_process ended with status {r.returncode}", returncode=1)
    assert r.returncode == 0, f"child exit status {r.returncode}"
