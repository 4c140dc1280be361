"""CPU tests (no GPU) of the fused range tracking / no-grad fake-quantisation route (engine.FUSED_RANGE_TRACK, csrc/range_track.hip,
DESIGN.md §4.23): the C entries refuse bad arguments on fake pointers before any launch, the workspace follows the block count
up to its cap, and the gate keeps the composition for what the kernels do not serve."""
import pytest
import torch

P = 0x10000                                                         # a fake, 16-byte aligned device pointer: nothing is launched


def _track(lib, x=P, rows=4, cols=8, ldx=8, mode=0, n_levels=256, range_in=P, zp_in=None, state=P, y=P, ws=P):
    return lib.qd_range_track(x, rows, cols, ldx, 0.95, 0.05, mode, n_levels, 0, 255, range_in, zp_in, state, y, ws, None)


def _plain(lib, x=P, rows=4, cols=8, ldx=8, delta=P, zp=P, y=P):
    return lib.qd_fakequant_rows(x, rows, cols, ldx, delta, zp, 0, 255, y, None)


@pytest.mark.parametrize("call,kw,word", [
    (_track, dict(x=None), "null pointer"), (_track, dict(range_in=None), "null pointer"), (_track, dict(state=None), "null pointer"),
    (_track, dict(ws=None), "null pointer"), (_track, dict(mode=2, zp_in=None), "null pointer"),
    (_track, dict(rows=0), "empty tensor"), (_track, dict(cols=0), "empty tensor"), (_track, dict(ldx=7), "row stride"),
    (_track, dict(n_levels=1), "n_levels"), (_track, dict(mode=3), "unknown mode"), (_track, dict(x=P + 2), "4-byte aligned"),
    (_track, dict(y=P + 4), "y must be 16-byte"), (_track, dict(ws=P + 8), "ws must be 16-byte"),
    (_plain, dict(x=None), "null pointer"), (_plain, dict(delta=None), "null pointer"), (_plain, dict(zp=None), "null pointer"),
    (_plain, dict(y=None), "null pointer"), (_plain, dict(rows=0), "empty tensor"), (_plain, dict(cols=0), "empty tensor"),
    (_plain, dict(ldx=7), "row stride"), (_plain, dict(x=P + 2), "4-byte aligned"), (_plain, dict(y=P + 4), "y must be 16-byte")])
def test_entries_refuse_bad_arguments_before_any_launch(call, kw, word):
    from qdiff import hip
    lib = hip.load()
    rc, msg = call(lib, **kw), lib.qd_last_error().decode()
    assert rc != 0 and word in msg and msg.startswith("qd_range_track" if call is _track else "qd_fakequant_rows"), (kw, msg)


def test_workspace_follows_the_block_count_up_to_the_cap():
    from qdiff import hip
    ws = hip.load().qd_range_track_ws_bytes
    chunk, cap = 2048, 2048                                         # elements a block takes per sweep; blocks at most
    assert [ws(1, 1), ws(1, chunk), ws(1, chunk + 1), ws(3, chunk)] == [16, 16, 32, 48]
    assert ws(1, chunk * cap) == ws(1, chunk * cap + 1) == ws(1 << 11, 1 << 20) == 16 * cap     # 2^31 elements: capped, not refused
    assert ws(0, 8) == ws(8, 0) == 0


@pytest.mark.parametrize("case", ["cpu", "fp16", "channel_wise", "knob_off"])
@pytest.mark.parametrize("tracking", [False, True])
def test_gate_keeps_the_composition(monkeypatch, case, tracking):
    """A wrong gate would hand a host tensor to hip._ptr, which raises; the counters stay where they were."""
    from qdiff import engine
    from qdiff.quant_layer import UniformAffineQuantizer
    x = torch.linspace(-1, 2, 4 * 6 * 5).reshape(4, 6, 5)
    q = UniformAffineQuantizer(n_bits=8, channel_wise=case == "channel_wise", scale_method='max', leaf_param=True)
    with torch.no_grad():
        want = q(x)
        if tracking:
            q.x_min, q.x_max = x.min(), x.max()                     # (a channel-wise initialisation records none)
        q.running_stat = tracking
        monkeypatch.setattr(engine, "FUSED_RANGE_TRACK", case != "knob_off")
        if case != "cpu":
            monkeypatch.setattr(engine, "mse_init_device_ok", lambda t: True)
        before = list(engine.RANGE_TRACK_CALLS)
        got = q(x.half() if case == "fp16" else x)
    assert engine.RANGE_TRACK_CALLS == before and got.shape == x.shape
    if not tracking and case != "fp16":
        assert torch.equal(got, want)
    if case == "knob_off":                                          # the one case the gate refuses by the knob alone
        engine.set_fused_range_track("1")
        assert engine.FUSED_RANGE_TRACK is True
        engine.set_fused_range_track(False)
        assert engine.FUSED_RANGE_TRACK is False
