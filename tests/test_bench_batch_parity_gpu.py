"""Whole quantised UNets at the evaluation batches bench.py measures (tests/bench_batch_cases.py).

Every other whole-model test runs two samples.  Here the fixture's two samples are replicated to the benchmark's batch, which
moves the convolutions onto the launch forms the benchmark runs (recorded per case through launch_forms and asserted to differ
from the batch-2 forms), and three statements are made of what the Python layer wires at that batch — plans and workspaces,
per-stream scratch, the attention workspace, the row groups of hip.temb_mlp, graph capture:

  replica   every output sample is bit-equal to the first replica of its source; positions 0 and 1 sit inside the envelope of
            test_quantised_unet_matches_reference against the reference golden and the fp64 oracle;
  replay    HIP-graph capture, two replays and the evaluation after invalidate_plans() equal the eager output bit for bit;
  pairs     8 and 5 classifier-free-guidance pairs: shared == unshared bit for bit, eager, captured and replayed.

The difference of positions 0 and 1 from the engine's own batch-2 output is RECORDED, not asserted: an epilogue that emits
GroupNorm statistics sums a 128-row chunk in tile order, the partial pass behind split-K in row order, so the launch form may
move a statistic by an ulp (profiles/bench_batch_parity.txt holds one run's figures, with the forms that account for them).

The models are built once per fixture and kept for the module (a case costs evaluations, not a pack).  Lines starting with
`[bench-batch]` (pytest -s) are the record the profile file is written from."""
import time

import pytest
import torch

import bench_batch_cases as BB
from conv_tall_tile_cases import launch_forms
from golden_util import fixture_inputs, load_fixture
from test_engine_models import _assert_envelope, _resume

pytestmark = pytest.mark.gpu

_MODELS = {}         # fixture name -> (fixture, resumed QuantModel)
_EAGER = {}          # (fixture name, batch) -> eager output of the replicated input, on the device


def _model(name, dev):
    if name not in _MODELS:
        t0 = time.perf_counter()
        fx = load_fixture(f"model_{name}.pt")
        _MODELS[name] = (fx, _resume(fx, dev))
        torch.cuda.synchronize()
        print(f"\n[bench-batch] {name}: model built in {time.perf_counter() - t0:.1f} s")
    return _MODELS[name]


def _call(qnn, x, t, c):
    with torch.no_grad():
        return (qnn(x, t, c) if c is not None else qnn(x, t)).clone()


def _inputs(fx, n, dev):
    return tuple(None if a is None else a.to(dev) for a in BB.replicate(fixture_inputs(fx, "test"), n))


def _eager(name, n, dev):
    """The eager output at batch n (graph replay off), computed once per case and left unchanged."""
    if (name, n) not in _EAGER:
        fx, qnn = _model(name, dev)
        qnn.enable_hip_graphs(False)
        y = _call(qnn, *_inputs(fx, n, dev))
        torch.cuda.synchronize()
        _EAGER[(name, n)] = y
    return _EAGER[(name, n)]


@pytest.fixture
def knob():
    from qdiff import engine
    before = engine.CFG_SHARE
    yield engine.set_cfg_share
    engine.set_cfg_share(before)


@pytest.mark.parametrize("name,n", BB.CASES, ids=[BB.case_id(c) for c in BB.CASES])
def test_replicas_are_bit_equal_and_inside_the_envelope(cuda, name, n):
    import qdiff
    from qdiff import hip
    fx, qnn = _model(name, cuda)
    t0 = time.perf_counter()
    qnn.enable_hip_graphs(False)
    mods = [m for m in qnn.modules() if isinstance(m, qdiff.QuantModule)]
    assert len(mods) == fx["n_quant_modules"] and all(m.int_ready() for m in mods)
    temb, real_temb = [], hip.temb_mlp

    def temb_spy(x, *a, **k):
        temb.append(tuple(x.shape))
        return real_temb(x, *a, **k)
    with launch_forms() as forms2:
        y2 = _call(qnn, *_inputs(fx, 2, cuda))
    hip.temb_mlp = temb_spy
    try:
        with launch_forms() as formsN:
            yN = _call(qnn, *_inputs(fx, n, cuda))
    finally:
        hip.temb_mlp = real_temb
    torch.cuda.synchronize()
    _EAGER.setdefault((name, n), yN)
    assert all(m._plan is not None for m in mods), "a QuantModule did not run the integer kernel"
    assert yN.shape[0] == n and torch.isfinite(yN).all()

    # the launch forms: what the batch is the parameter of
    c2, cN = BB.form_counts(forms2), BB.form_counts(formsN)
    new = [f for f, _ in cN if f not in dict(c2)]
    print(f"\n[bench-batch] {name} batch 2: {len(forms2)} launches: {BB.forms_line(c2)}")
    print(f"[bench-batch] {name} batch {n}: {len(formsN)} launches: {BB.forms_line(cN)}")
    print(f"[bench-batch] {name} batch {n}: forms batch 2 did not run: {new}; hip.temb_mlp inputs {sorted(set(temb))}")
    assert new, f"batch {n} ran only the launch forms of batch 2: {cN}"
    if (name, n) == ("sd_full", 16):
        assert any(f[0] == 256 for f, _ in cN), f"no 256-row tile at the benchmark's batch: {cN}"
    if (name, n) == ("ldm_full", 64):
        # more rows than one launch of qd_temb_mlp holds (hip.temb_mlp: 44 KiB of fp32 words): the row-group split ran
        assert any(B == n and B * K > 44 * 1024 for B, K in temb), temb

    # replicas
    msg = BB.replica_mismatch(yN)
    assert msg is None, f"{name} batch {n}: {msg}"

    # cross-batch record (no assertion: module docstring)
    y01 = yN[:2].float().cpu()
    rng = fx["out_wa"].abs().max().item()
    dx = (y01 - y2.float().cpu()).abs()
    print(f"[bench-batch] {name} batch {n} vs batch 2, positions 0 and 1: {int((dx != 0).sum())} of {dx.numel()} elements differ, "
          f"max {dx.max().item() / rng:.3e} of range")

    # positions 0 and 1 are the fixture's two samples
    assert BB.thue_morse(n)[:2] == [0, 1]
    _assert_envelope(f"{name} batch {n}", y01, fx)
    print(f"[bench-batch] {name} batch {n}: replica test {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name,n", BB.CASES, ids=[BB.case_id(c) for c in BB.CASES])
def test_graph_replay_and_recapture_equal_eager(cuda, name, n):
    fx, qnn = _model(name, cuda)
    want = _eager(name, n, cuda)
    t0 = time.perf_counter()
    x, t, c = _inputs(fx, n, cuda)
    qnn.enable_hip_graphs(True)
    try:
        if c is not None:
            with torch.no_grad():                          # (prepare_context declines while autograd is on)
                assert qnn.prepare_context(c)
        got = {"capture": _call(qnn, x, t, c)}
        assert len(qnn._graphs) == 1
        got["replay 1"] = _call(qnn, x, t, c)
        got["replay 2"] = _call(qnn, x, t, c)
        assert len(qnn._graphs) == 1
        qnn.invalidate_plans()                             # packs, plans, prepared contexts and graphs go; everything is rebuilt
        assert qnn._graphs == {}
        got["after invalidate_plans"] = _call(qnn, x, t, c)
        assert len(qnn._graphs) == 1
        got["replay after invalidate_plans"] = _call(qnn, x, t, c)
    finally:
        qnn.enable_hip_graphs(False)
    torch.cuda.synchronize()
    for what, y in got.items():
        assert torch.equal(y, want), (f"{name} batch {n}, {what}: {int((y != want).sum())} elements differ from the eager output, "
                                      f"max |diff| {(y - want).abs().max().item():.3e}; replicas: {BB.replica_mismatch(y)}")
    print(f"\n[bench-batch] {name} batch {n}: replay test {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name,n", BB.PAIR_CASES, ids=[f"{a}-{b}pairs" for a, b in BB.PAIR_CASES])
def test_guidance_pairs_shared_equals_unshared(cuda, name, n, knob):
    """test_cfg_pair_gpu.py::test_shared_evaluation_equals_unshared at the benchmark's pair counts: residual row period and
    query head period with n groups of rows instead of one."""
    from qdiff import engine
    fx, qnn = _model(name, cuda)
    t0 = time.perf_counter()
    xh, th, ctx = BB.pair_inputs(fixture_inputs(fx, "test"), n, cuda)
    x2, t2 = torch.cat([xh, xh]), torch.cat([th, th])
    g = torch.Generator(device=cuda).manual_seed(5)
    xd = torch.cat([xh, torch.randn(xh.shape, device=cuda, generator=g)])           # 2n distinct samples
    td = torch.cat([th, (th + 7) % 1000])
    qnn.enable_hip_graphs(False)
    try:
        knob(False)
        want = _call(qnn, x2, t2, ctx)
        want_distinct = _call(qnn, xd, td, ctx)
        p0 = qnn.pair_evals
        knob(True)
        with torch.no_grad():
            assert qnn.prepare_context(ctx)
        assert engine.mark_pair(x2, t2)
        eager = _call(qnn, x2, t2, ctx)
        assert qnn.pair_evals == p0 + 1
        distinct = _call(qnn, xd, td, ctx)                                           # no mark: evaluated unshared
        assert qnn.pair_evals == p0 + 1
        qnn.enable_hip_graphs(True)
        g1 = _call(qnn, x2, t2, ctx)                                                 # captures the shared evaluation
        g2 = _call(qnn, x2, t2, ctx)                                                 # replays it
        assert qnn.pair_evals == p0 + 3
        g3 = _call(qnn, xd, td, ctx)                                                 # the unshared graph
        assert qnn.pair_evals == p0 + 3
    finally:
        qnn.enable_hip_graphs(False)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and not torch.equal(want[:n], want[n:])       # the halves' contexts differ
    for what, y in (("eager", eager), ("capture", g1), ("replay", g2)):
        assert torch.equal(y, want), (f"{name}, {n} pairs, shared {what}: {int((y != want).sum())} elements differ from the unshared "
                                      f"evaluation, max |diff| {(y - want).abs().max().item():.3e}; first sample that differs: "
                                      f"{next(i for i in range(2 * n) if not torch.equal(y[i], want[i]))}")
    assert torch.equal(distinct, want_distinct) and torch.equal(g3, want_distinct)
    print(f"\n[bench-batch] {name} {n} pairs: pair test {time.perf_counter() - t0:.2f} s")
