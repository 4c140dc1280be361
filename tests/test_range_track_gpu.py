"""GPU tests of the fused range tracking / no-grad fake-quantisation route (engine.FUSED_RANGE_TRACK, csrc/range_track.hip, DESIGN.md
§4.23).  The reference is the composition itself: the same UniformAffineQuantizer, deep-copied, run with the knob off on the same
tensor.  y, x_min, x_max, delta and zero_point must agree bit for bit (NaN positions, not payloads)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = {"affine8": dict(n_bits=8), "always_zero16": dict(n_bits=16, always_zero=True), "symmetric8": dict(n_bits=8, symmetric=True)}
# the smallest sizes at which each path can go wrong: one element; a scalar tail only; a second block and a tail; one element past
# the single sweep of the 2048 blocks (the grid-stride loop runs twice); the two halves of a split input: rows of 75 and 100
# floats that start off 16 bytes, the other half lying in the gaps
SHAPES = {"n1": (1, None), "n3": (3, None), "n1025": (256 * 4 + 1, None), "sweep": (2048 * 2048 + 1, None),
          "slice_lo": ((3, 7, 5, 5), slice(0, 3)), "slice_hi": ((3, 7, 5, 5), slice(3, 7))}


def _draw(dev, shape, cut, seed, positive, plant="first"):
    """A continuous draw (no signed-zero ties) with the extremes planted; for a slice, larger values fill the gap."""
    g = torch.Generator(device=dev).manual_seed(seed)
    full = torch.rand(shape, generator=g, device=dev) * 1.5 + (0.01 if positive else -0.7)
    x = full if cut is None else full[:, cut]
    if cut is not None:
        full[:, :cut.start], full[:, cut.stop:] = 1e6, -1e6
    rows, cols = (1, x.numel()) if cut is None else (x.shape[0], x[0].numel())
    top = {"first": 0, "last": rows * cols - 1, "row_last": cols - 1}[plant]
    flat = x.reshape(rows, cols) if cut is None else x.flatten(1)        # (views: x stays what the quantiser is handed)
    flat[top // cols, top % cols] = 7.0
    if rows * cols > 1:
        bottom = rows * cols - 1 - top if plant != "row_last" else (cols if rows > 1 else 0)
        flat[bottom // cols, bottom % cols] = 0.001 if positive else -7.0
    return x


def _quantizer(dev, mode):
    from qdiff.quant_layer import UniformAffineQuantizer
    q = UniformAffineQuantizer(scale_method='max', leaf_param=True, **MODES[mode])
    with torch.no_grad():
        q(_draw(dev, 64, None, 1, "always_zero" in mode))               # data-dependent initialisation, knob off
    return q


def _bits(t, dev):
    t = torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int32)


def _both(q, x, which):
    """Run q (knob on) and its deep copy (knob off) on x; the route must have been taken; everything must agree bit for bit."""
    from qdiff import engine
    ref = copy.deepcopy(q)
    before = list(engine.RANGE_TRACK_CALLS)
    with torch.no_grad():
        want = ref(x)
        engine.set_fused_range_track(True)
        try:
            got = q(x)
        finally:
            engine.set_fused_range_track(False)
    after = list(engine.RANGE_TRACK_CALLS)
    assert after[which] == before[which] + 1 and after[1 - which] == before[1 - which]
    assert got.shape == want.shape and torch.equal(_bits(got, x.device), _bits(want, x.device))
    for name in ("x_min", "x_max", "delta", "zero_point"):
        a, b = getattr(q, name), getattr(ref, name)
        assert type(a) is type(b) and torch.equal(_bits(a, x.device), _bits(b, x.device)), (name, a, b)
        assert not torch.is_tensor(a) or (a.shape == b.shape and a.dtype == b.dtype and a.device == b.device), name
    return got


@pytest.mark.parametrize("plant", ["first", "last", "row_last"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", list(MODES))
def test_tracked_call_is_the_composition(cuda, mode, shape, plant):
    q = _quantizer(cuda, mode)
    q.running_stat = True
    _both(q, _draw(cuda, *SHAPES[shape], 2, "always_zero" in mode, plant), 0)


@pytest.mark.parametrize("zp_tensor", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", list(MODES))
def test_plain_call_is_the_composition(cuda, mode, shape, zp_tensor):
    q = _quantizer(cuda, mode)
    assert isinstance(q.zero_point, int)                                # 'max' leaves a host integer
    if zp_tensor:
        q.zero_point = torch.tensor(float(q.zero_point), device=cuda)
    _both(q, _draw(cuda, *SHAPES[shape], 3, "always_zero" in mode), 1)


@pytest.mark.parametrize("shape", ["n1025", "slice_hi"])
@pytest.mark.parametrize("mode", list(MODES))
def test_state_chains_over_three_calls(cuda, mode, shape):
    q = _quantizer(cuda, mode)
    q.running_stat = True
    for seed in (4, 5, 6):
        _both(q, _draw(cuda, *SHAPES[shape], seed, "always_zero" in mode, "last"), 0)
    assert q.x_min.data_ptr() + 4 == q.x_max.data_ptr()                 # views of one state tensor, handed back in place


@pytest.mark.parametrize("mode,c", [("affine8", 0.5), ("always_zero16", 0.0), ("symmetric8", 0.0)])
def test_constant_tensor_at_the_old_range_hits_the_delta_floor(cuda, mode, c):
    q = _quantizer(cuda, mode)
    q.running_stat = True
    q.x_min, q.x_max = torch.tensor(c, device=cuda), torch.tensor(c, device=cuda)
    _both(q, torch.full((5, 13), c, device=cuda), 0)
    assert float(q.delta) == float(torch.tensor(1e-8, dtype=torch.float32))


@pytest.mark.parametrize("tracking", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_nan_element(cuda, mode, tracking):
    q = _quantizer(cuda, mode)
    q.running_stat = tracking
    x = _draw(cuda, 256 * 4 + 1, None, 7, "always_zero" in mode)
    x[517] = float("nan")
    y = _both(q, x, 0 if tracking else 1)
    assert bool(torch.isnan(y).all()) if tracking else torch.isnan(y).nonzero().flatten().tolist() == [517]
