"""CPU tests (no GPU) of the classifier-free-guidance pair route: an evaluation whose batch halves hold the same
samples runs input_blocks[1] up to its first cross-attention once, the three launches after the fork read the half-batch
operands periodically (qd_conv_desc.res_period, qd_attn_i8_qp), and everything the integer route refuses evaluates as always.
Host logic on tests/cfg_pair_emulator.py (tests/abi_emulator.py plus the two periods)."""
import ctypes
import os
import re
import tempfile

import pytest
import torch

import cfg_pair_emulator
from golden_util import build_ckpt, build_engine_model, fixture_inputs, load_fixture, quant_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def emu(monkeypatch):
    from qdiff import engine
    monkeypatch.setattr(engine, "CFG_SHARE", True)
    return cfg_pair_emulator.install(monkeypatch)


def _resume_cpu(fx):
    import qdiff
    from qdiff.utils import resume_cali_model
    spec = fx["spec"]
    wq, aq = quant_params(spec)
    qnn = qdiff.QuantModel(build_engine_model(spec), wq, aq, sm_abit=spec["sm_abit"]).eval()
    cal = tuple(a for a in fixture_inputs(fx, "cal") if a is not None)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ckpt.pth")
        torch.save(build_ckpt(fx), path)
        resume_cali_model(qnn, path, cal, quant_act=True, cond=spec["ctx"] is not None)
    qnn.set_quant_state(True, True)
    return qnn


def _warm(qnn, x, t, c):
    """The conditioning prepared up front, as a sampling run has it from its second evaluation on: the call lists below then
    hold the evaluation alone, not the once-per-run to_k / to_v chain."""
    from qdiff import engine
    on = engine.CFG_SHARE
    engine.set_cfg_share(False)
    try:
        with torch.no_grad():
            qnn(x, t, c) if c is not None else qnn(x, t)          # plans, packs, the state token
    finally:
        engine.set_cfg_share(on)
    if c is not None:
        with torch.no_grad():
            assert qnn.prepare_context(c)


def _pair_inputs(fx, n=1):
    """x, t of n samples duplicated the way a sampler does, and a context of 2n distinct rows (uncond | cond)."""
    x, t, c = fixture_inputs(fx, "test")
    x, t = x[:1].repeat(n, 1, 1, 1) + torch.arange(n).view(n, 1, 1, 1) * 0.25, t[:1].repeat(n) + torch.arange(n)
    g = torch.Generator().manual_seed(7)
    ctx = torch.randn((2 * n,) + tuple(c.shape[1:]), generator=g) if c is not None else None
    return torch.cat([x] * 2), torch.cat([t] * 2), ctx


def _eval(qnn, calls, x, t, c, mark=True):
    from qdiff import engine
    if mark:
        engine.mark_pair(x, t)
    del calls[:]
    before = qnn.pair_evals
    with torch.no_grad():
        y = qnn(x, t, c) if c is not None else qnn(x, t)
    return y, list(calls), qnn.pair_evals - before


@pytest.fixture(scope="module")
def sd_tiny():
    return load_fixture("model_sd_tiny.pt")


@pytest.mark.parametrize("n", [1, 2])
def test_marked_pair_shares_the_stretch_and_changes_no_byte(emu, sd_tiny, n):
    """sd_tiny (x 4 x 16 x 16, context 7 x 48), n samples duplicated and marked: the launches of the shared stretch carry batch n,
    exactly three launches carry a period, and the output equals the knob-off output bit for bit."""
    from qdiff import engine
    qnn = _resume_cpu(sd_tiny)
    x, t, c = _pair_inputs(sd_tiny, n)
    _warm(qnn, x, t, c)
    T = x.shape[2] * x.shape[3]
    engine.set_cfg_share(False)
    y_off, calls_off, took = _eval(qnn, emu, x, t, c)
    assert took == 0 and not any(k[0] == "conv" and k[3] for k in calls_off) and all(k[1] == k[2] for k in calls_off if k[0] == "attn")
    engine.set_cfg_share(True)
    y_on, calls_on, took = _eval(qnn, emu, x, t, c)
    assert took == 1
    assert torch.equal(y_on, y_off)
    assert len(calls_on) == len(calls_off)                       # the same launches, some of them on half the rows
    diff = [(a, b) for a, b in zip(calls_off, calls_on) if a != b]
    periodic = [b for _, b in diff if (b[0] == "conv" and b[3]) or (b[0] == "attn" and b[2] != b[1])]
    # the fork: attn2 (2n samples' heads on n samples' queries), attn2.to_out and proj_out (2n T rows, period n T)
    heads = periodic[0][1] // (2 * n)
    assert periodic == [("attn", 2 * n * heads, n * heads, T, c.shape[1]), ("conv", 2 * n * T, periodic[1][2], n * T),
                        ("conv", 2 * n * T, periodic[2][2], n * T)]
    shared = [(a, b) for a, b in diff if b not in periodic]
    assert shared and all(a[0] == b[0] and b[1] * 2 == a[1] and a[2:] == b[2:] or (a[0] == "attn" and b[1] * 2 == a[1] and b[2] * 2 == a[2])
                          for a, b in shared), shared
    # the first self-attention ran on n samples
    assert ("attn", n * heads, n * heads, T, T) in calls_on and ("attn", 2 * n * heads, 2 * n * heads, T, T) in calls_off
    # everything after the fork, and conv_in before it, is untouched
    first = calls_off.index(diff[0][0])
    last = len(calls_off) - 1 - calls_off[::-1].index(diff[-1][0])
    assert calls_on[:first] == calls_off[:first] and calls_on[last + 1:] == calls_off[last + 1:] and first >= 1


def _unshared(qnn, emu, x, t, c, want_calls, want_y, mark=True):
    y, calls, took = _eval(qnn, emu, x, t, c, mark=mark)
    assert took == 0 and calls == want_calls
    if want_y is not None:
        assert torch.equal(y, want_y)


def test_everything_else_evaluates_as_always(emu, sd_tiny):
    """Unmarked input, an in-place write after marking, an odd batch, a context of another batch, the knob, a foreign hook:
    the call list is the unshared one."""
    from qdiff import engine
    qnn = _resume_cpu(sd_tiny)
    x, t, c = _pair_inputs(sd_tiny, 1)
    _warm(qnn, x, t, c)
    engine.set_cfg_share(False)
    y_off, calls_off, _ = _eval(qnn, emu, x, t, c)
    engine.set_cfg_share(True)
    from qdiff import quant_block as qb
    pin = qb._CTX_PIN
    try:
        qb._CTX_PIN = False                                      # (no prepared context: no by-value match that could carry a probe)
        _unshared(qnn, emu, x.clone(), t.clone(), c, calls_off, y_off, mark=False)            # unmarked
        x2, t2 = x.clone(), t.clone()
        engine.mark_pair(x2, t2)
        x2.add_(0.0)                                                                          # in-place write after marking
        _unshared(qnn, emu, x2, t2, c, calls_off, y_off, mark=False)
    finally:
        qb._CTX_PIN = pin
    # knob off
    engine.set_cfg_share(False)
    _unshared(qnn, emu, x, t, c, calls_off, y_off)
    engine.set_cfg_share(True)
    # a foreign hook anywhere below the model
    h = qnn.model.out.register_forward_hook(lambda m, a, o: None)
    _unshared(qnn, emu, x, t, c, calls_off, y_off)
    h.remove()
    assert _eval(qnn, emu, x, t, c)[2] == 1                       # ... and with the hook gone the pair is shared again
    # odd batch
    x3, t3, c3 = torch.cat([x, x[:1]]), torch.cat([t, t[:1]]), torch.cat([c, c[:1]])
    assert not engine.mark_pair(x3, t3)
    y3, calls3, took = _eval(qnn, emu, x3, t3, c3, mark=False)
    assert took == 0 and not any(k[0] == "conv" and k[3] for k in calls3)
    # a context of another batch: never a pair.  The evaluation fails as it always did (operands of one sample, latents of two),
    # and what it launched until then is what the unshared evaluation launches: no period, no half batch
    engine.mark_pair(x, t)
    before = qnn.pair_evals
    del emu[:]
    with pytest.raises(Exception) as err:
        with torch.no_grad():
            qnn(x, t, c[:1])
    assert "guidance pair" not in str(err.value)
    got = [k for k in emu if not (k[0] == "conv" and k[1] == c.shape[1])]       # (without the to_k / to_v chain of the new context: 7 rows)
    assert qnn.pair_evals == before and got and got == calls_off[:len(got)]


def test_other_layouts_are_not_shared(emu):
    """ldm_tiny has no SpatialTransformer behind its first residual block: a marked pair evaluates as always."""
    from qdiff import engine
    fx = load_fixture("model_ldm_tiny.pt")
    qnn = _resume_cpu(fx)
    x, t, c = _pair_inputs(fx, 1)
    engine.set_cfg_share(False)
    y_off, calls_off, _ = _eval(qnn, emu, x, t, c)
    engine.set_cfg_share(True)
    _unshared(qnn, emu, x, t, c, calls_off, y_off)


def test_unmarked_pair_rides_in_the_context_match_read_back(emu, sd_tiny, monkeypatch):
    """The unmodified sampler marks nothing and builds fresh tensors at every step: when ContextKV.match reads its by-value flags
    back anyway, "the halves are equal" travels in that ONE .tolist(); a marked pair costs no read-back at all."""
    from qdiff import engine
    qnn = _resume_cpu(sd_tiny)
    x, t, c = _pair_inputs(sd_tiny, 1)
    reads = []
    real_tolist, real_item = torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append("tolist"), real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (reads.append("item"), real_item(self))[1])
    _warm(qnn, x, t, c)
    del reads[:]
    assert _eval(qnn, emu, x, t, c)[2] == 1 and reads == []      # marked, same context object: nothing is read back
    del reads[:]
    engine.set_cfg_share(False)
    _eval(qnn, emu, x.clone(), t.clone(), c.clone(), mark=False)
    base = list(reads)                                            # the by-value match of a fresh context: what the parent reads back
    engine.set_cfg_share(True)
    del reads[:]
    y, calls, took = _eval(qnn, emu, x.clone(), t.clone(), c.clone(), mark=False)
    assert took == 1 and reads == base                             # (on a GPU `base` is the ONE .tolist() of ContextKV.match)
    del reads[:]
    xd = x.clone()
    xd[1] += 1.0                                                  # halves differ: the probe says no
    assert _eval(qnn, emu, xd, t.clone(), c.clone(), mark=False)[2] == 0 and reads == base


def test_inference_tensors_are_never_marked():
    from qdiff import engine
    with torch.inference_mode():
        x, t = torch.zeros(2, 4, 8, 8), torch.zeros(2, dtype=torch.long)
    assert not engine.mark_pair(x, t) and not engine.pair_marked(x, t)
    x, t = torch.zeros(2, 4, 8, 8), torch.zeros(2, dtype=torch.long)
    assert engine.mark_pair(x, t) and engine.pair_marked(x, t)
    t.add_(1)
    assert not engine.pair_marked(x, t)


def test_guided_eps_marks_its_doubled_batch(emu, sd_tiny):
    from qdiff import engine, sampling
    qnn = _resume_cpu(sd_tiny)
    x, t, c = fixture_inputs(sd_tiny, "test")
    x, t, cond, uncond = x[:1], t[:1], c[:1], c[1:2]
    outs = []
    for on in (False, True):
        engine.set_cfg_share(on)
        before = qnn.pair_evals
        with torch.no_grad():
            outs.append(sampling.guided_eps(qnn, x, t, cond, uncond, 7.5))
        assert qnn.pair_evals - before == (1 if on else 0)
    assert torch.equal(outs[0], outs[1])


def test_header_and_ctypes_agree_on_the_new_entries():
    """res_period sits where _pad3 sat (the offset test of tests/test_host_logic.py covers the layout); qd_attn_i8_qp is qd_attn_i8
    plus one int."""
    from qdiff import hip
    names = [n for n, _ in hip.ConvDesc._fields_]
    assert names[-1] == "res_period" and names[-2] == "upsample2x" and "_pad3" not in names
    assert hip.ConvDesc.res_period.offset == ctypes.sizeof(hip.ConvDesc) - 4
    header = open(os.path.join(ROOT, "include", "qdiff_hip.h")).read()

    def nargs(fn):
        m = re.search(r"\bint\s+" + fn + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        return len([a for a in m.group(1).split(",") if a.strip()])
    assert nargs("qd_attn_i8_qp") == nargs("qd_attn_i8") + 1 == 31
    assert "qd_attn_i8_qp" in hip.EXPORTS
    lib = hip.load()
    assert len(lib.qd_attn_i8_qp.argtypes) == len(lib.qd_attn_i8.argtypes) + 1 == 31
    assert re.search(r"#define\s+QD_ABI_VERSION\s+20\b", header)
