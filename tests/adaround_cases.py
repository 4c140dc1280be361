"""Shared by tests/test_adaround_fused_gpu.py and tests/test_adaround_fused_host.py: the cases of the fused AdaRound route
(engine.FUSED_ADAROUND), the fp64 evaluation both the fused route and the fp32 torch composition are judged
against, and the comparison itself.

Units of the errors (the bound is RELATIVE: fused worst <= 2 x composition worst, same case, same unit):
  * w_hat:   delta of the row (the error in code units);
  * galpha:  per element |gw * delta| + |greg * b * 2 * v^(b-1)|, the magnitudes of the two chains before the factors <= 1.2;
  * reg_sum: the sum of the term magnitudes |1 - v^b|.
The composition's figure is replaced by HALF_ULP = 2^-24 of the unit, the rounding of one fp32 operation, in two places only:
  * for w_hat and galpha (maxima over the elements) where it is exactly 0 — it hit the fp64 value, as the single-element case can:
    2 x 0 would demand bit-equality with fp64, which no fp32 evaluation promises;
  * for reg_sum, ONE fp32 scalar, where it is below HALF_ULP: the final rounding of the scalar alone is up to 2^-24 of its
    magnitude, and where the composition's sum lands inside that is chance (measured on the MI355X, (40,96) at b = 7.3:
    composition 1.8e-8, its summation errors cancelling, against 8.4e-8 for the CORRECTLY ROUNDED sum of the same fp32 terms,
    which is what the route returns — the kernel adds the terms in fp64 and the total is rounded once; on the host,
    (5,1031) at b = 20: 1.5e-8 against 5.3e-8).  No fp32 scalar can promise less.
"""
import math

import torch

HALF_ULP = 2.0 ** -24
NEAR = 2.0 ** -20            # distance from a decision boundary below which galpha is not compared element by element
GAMMA, ZETA = -0.1, 1.1
LOG11 = math.log(11.0)       # sigmoid(+-log 11) * 1.2 - 0.1 = 1 resp. 0: hr on the clamp boundary


def make_quantizer(w, bits, seed, planted=()):
    """AdaRoundQuantizer with soft targets over `w` (a weight tensor or a channel slice of one): channel-wise 'max' grid with
    delta shrunk by 0.8 (codes clamp at both ends), alpha spread so that part of the soft targets saturate, `planted` written
    over the first elements of alpha."""
    from qdiff.adaptive_rounding import AdaRoundQuantizer
    from qdiff.quant_layer import UniformAffineQuantizer
    uaq = UniformAffineQuantizer(n_bits=bits, channel_wise=True, scale_method='max')
    uaq.ensure_init(w)
    uaq.delta = uaq.delta * 0.8
    q = AdaRoundQuantizer(uaq=uaq, round_mode='learned_hard_sigmoid', weight_tensor=w)
    q.soft_targets = True
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        a = q.alpha.detach().cpu()
        a = a * 1.5 + torch.randn(a.shape, generator=g)
        flat = a.reshape(-1)
        for i, v in enumerate(planted[:flat.numel()]):
            flat[i] = v
        q.alpha.copy_(a.to(q.alpha.device))
    return q


def weights(shape, seed, device):
    """Random weights with one outlier channel (very different delta per row)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * 0.1
    if shape[0] > 1:
        w[shape[0] // 2] *= 40.0
    return w.to(device)


def reference64(w, q, b, gw, greg):
    """fp64 evaluation of the header's formulas on the fp32 floor(w / delta)."""
    rows = w.shape[0]
    w2 = w.detach().reshape(rows, -1)
    d32, z32 = q.delta.detach().reshape(rows, 1).float(), q.zero_point.detach().reshape(rows, 1).float()
    base = torch.floor(w2 / d32).double()
    d, z, a = d32.double(), z32.double(), q.alpha.detach().reshape(rows, -1).double()
    top = float(q.n_levels - 1)
    zg = float(torch.tensor(ZETA - GAMMA, dtype=torch.float32))       # the fp32 scalar both fp32 routes multiply by
    s = 1 / (1 + torch.exp(-a))
    hr = s * zg + GAMMA
    h = hr.clamp(0, 1)
    c = base + h + z
    out = dict(w_hat=(c.clamp(0, top) - z) * d, hr=hr, h=h, c=c, delta=d.expand_as(a), top=top)
    m_h = ((hr >= 0) & (hr <= 1)).double()
    m_c = ((c >= 0) & (c <= top)).double()
    tail = zg * (1 - s) * s
    out["rec"] = gw.detach().reshape(rows, -1).double() * d * tail            # before the two masks
    out["unit"] = (gw.detach().reshape(rows, -1).double() * d).abs()
    out["reg"] = torch.zeros_like(a)
    out["reg_sum"] = out["reg_mag"] = None
    if b is not None:
        u = h - 0.5
        v = u.abs() * 2
        out["reg"] = -float(greg) * b * v.pow(b - 1) * 2 * torch.sign(u) * tail
        out["unit"] = out["unit"] + abs(float(greg)) * b * 2 * v.pow(b - 1)
        out["reg_sum"] = (1 - v.pow(b)).sum()
        out["reg_mag"] = (1 - v.pow(b)).abs().sum()
    out["m_h"], out["m_c"] = m_h, m_c
    out["galpha"] = m_h * (m_c * out["rec"] + out["reg"])
    soft = (h > 0) & (h < 1)
    near_h = (hr.abs() < NEAR) | ((hr - 1).abs() < NEAR)
    near_c = soft & ((c.abs() < NEAR) | ((c - top).abs() < NEAR))
    out["near"] = near_h | near_c
    out["saturated"] = ~soft
    return out


def run_route(q, w, b, gw, greg, fused):
    """(w_hat, reg_sum or None, alpha.grad) of loss = sum(w_hat * gw) + greg * reg_sum through the fused route or the composition.
    w_hat enters the loss as the first half of a torch.cat along the channels, as the half of a split layer does: its gradient
    arrives as a channel slice (row stride 2 x cols) holding exactly gw."""
    from qdiff import engine
    q.alpha.grad = None
    prev = engine.FUSED_ADAROUND
    engine.set_fused_adaround(fused)
    try:
        if fused:
            q.__dict__['_reg_b'] = b
        with torch.enable_grad():
            w_hat = q(w)
            reg = None
            if b is not None:
                if fused:
                    assert q.__dict__['_reg_sum'][0] == b
                    reg = q.__dict__['_reg_sum'][1]
                else:
                    reg = (1 - ((q.get_soft_targets() - .5).abs() * 2).pow(b)).sum()
            loss = (torch.cat([w_hat, w_hat.detach()], dim=1) * torch.cat([gw, gw], dim=1)).sum()
            if reg is not None:
                loss = loss + greg * reg
            loss.backward()
    finally:
        engine.set_fused_adaround(prev)
        q.__dict__.pop('_reg_b', None)
        q.__dict__.pop('_reg_sum', None)
    g = q.alpha.grad.detach().clone()
    q.alpha.grad = None
    return w_hat.detach(), (None if reg is None else reg.detach()), g


def errors(ref, w_hat, reg, galpha):
    """Worst errors against the fp64 evaluation, in the units of the module docstring (CPU doubles)."""
    shape = ref["hr"].shape
    w_hat, galpha = w_hat.detach().cpu().double().reshape(shape), galpha.detach().cpu().double().reshape(shape)
    assert torch.isfinite(w_hat).all() and torch.isfinite(galpha).all()
    e = dict(w_hat=((w_hat - ref["w_hat"]).abs() / ref["delta"]).max().item())
    keep = ~ref["near"] & (ref["unit"] > 0)
    ge = (galpha - ref["galpha"]).abs()[keep] / ref["unit"][keep]
    e["galpha"] = ge.max().item() if ge.numel() else 0.0
    # on a boundary: the mask passes the gradient or blocks it — one of the legitimate outcomes, nothing in between
    nr = ref["near"]
    if nr.any():
        outcomes = torch.stack([torch.zeros_like(ref["rec"]), ref["reg"], ref["rec"] + ref["reg"]])[:, nr]
        miss = (outcomes - galpha[nr]).abs().min(0).values
        assert (miss <= 2.0 ** -12 * ref["unit"][nr] + 1e-30).all(), "a boundary element took neither legitimate value"
    if reg is not None:
        assert math.isfinite(float(reg))
        e["reg_sum"] = abs(float(reg) - float(ref["reg_sum"])) / max(float(ref["reg_mag"]), 1e-300)
    return e


def judge(q, w, b, gw, greg, report=None, label=""):
    """Test 1 of the issue for one case: both routes against fp64; returns (fused errors, composition errors)."""
    ref = reference64(w.cpu(), _cpu_view(q), b, gw.cpu(), greg)
    share = ref["near"].double().mean().item()
    assert share <= 0.02, f"{label}: {share:.3%} of the elements lie on a decision boundary"
    c_w, c_reg, c_g = run_route(q, w, b, gw, greg, fused=False)
    f_w, f_reg, f_g = run_route(q, w, b, gw, greg, fused=True)
    sat = (ref["saturated"] & ~ref["near"]).reshape(f_w.shape)     # (on the boundary itself fp32 may still call h soft)
    assert sat.any() or w.numel() < 16, f"{label}: no saturated soft target in this case"
    assert torch.equal(f_w.cpu()[sat], c_w.cpu()[sat]), f"{label}: w_hat differs where h is saturated (decisions only)"
    assert (f_g.cpu()[sat] == 0).all(), f"{label}: a saturated element received a gradient"
    ef, ec = errors(ref, f_w, f_reg, f_g), errors(ref, c_w, c_reg, c_g)
    line = f"[adaround {label} b={b}] " + ", ".join(f"{k}: fused {ef[k]:.3e} composition {ec[k]:.3e}" for k in ef) \
        + f", bit-equal w_hat={torch.equal(f_w, c_w)} galpha={torch.equal(f_g, c_g)}, boundary share {share:.2%}"
    print(line)
    if report is not None:
        report.append(line)
    assert_within(ef, ec, f"{label} b={b}")
    return ef, ec, ref


def assert_within(ef, ec, label):
    """The issue's bound: the fused route's worst error at most 2 x the composition's, per unit (module docstring)."""
    for k in ef:
        floor = HALF_ULP if (k == "reg_sum" or ec[k] == 0) else 0.0
        assert ef[k] <= 2 * max(ec[k], floor), f"{label}: {k} fused {ef[k]:.3e} > 2 x composition {ec[k]:.3e}"


class Upstream:
    """Forward hook on an AdaRoundQuantizer inside a module: keeps the weight (slice) it was called on, its output w_hat and the
    gradient autograd delivers there, so that a whole-module run can be judged per element exactly as judge() does."""

    def __init__(self, q):
        self.w = self.w_hat = self.gw = None
        self.handle = q.register_forward_hook(self._seen)

    def _seen(self, mod, inputs, out):
        self.w, self.w_hat, self.gw = inputs[0].detach(), out.detach(), None
        if out.requires_grad:
            out.register_hook(self._grad)

    def _grad(self, g):
        self.gw = g.detach().clone()

    def errors(self, q, b, greg):
        """errors() of what this hook saw in the last forward / backward; alpha.grad is the quantiser's."""
        ref = reference64(self.w.cpu(), _cpu_view(q), b, self.gw.cpu(), greg)
        assert ref["near"].double().mean().item() <= 0.02
        return errors(ref, self.w_hat, None, q.alpha.grad)


class _cpu_view:
    """The quantiser's tensors on the host, for reference64."""

    def __init__(self, q):
        self.delta, self.zero_point, self.alpha, self.n_levels = q.delta.cpu(), q.zero_point.cpu(), q.alpha.detach().cpu(), q.n_levels
