"""AdaRound weight quantiser (https://arxiv.org/abs/2004.10568) — counterpart of the reference's
qdiff/adaptive_rounding.py with the same constructor, attributes (`alpha`, `delta`, `zero_point`,
`soft_targets`, `n_levels`, `round_mode`, ...) and state-dict keys.

At inference (round_mode='learned_hard_sigmoid', soft_targets=False) the codes are
    W = clamp(floor(w/delta) + (alpha >= 0) + zero_point, 0, n_levels-1)
(reference adaptive_rounding.py:49-59).  The integer engine evaluates that formula once, inside
qd_pack_weights (csrc/quantize.hip), instead of on every forward; `forward` below is the
differentiable fp32 simulation that calibration (block/layer reconstruction) optimises through.
"""
import logging

import torch
from torch import nn

from .quant_layer import UniformAffineQuantizer, round_ste

logger = logging.getLogger(__name__)


class FusedAdaRound(torch.autograd.Function):
    """(w_hat, reg_sum) of a soft-target 'learned_hard_sigmoid' quantiser as ONE HIP launch forward and ONE backward
    (csrc/adaround.hip) instead of the ~45 elementwise kernels autograd runs for AdaRoundQuantizer.forward plus the
    regulariser's second get_soft_targets() (reference adaptive_rounding.py:39-74, block_recon.py:217-229).  reg_sum is
    sum(1 - |2 h - 1|^reg_b) (an unused, non-differentiable scalar when reg_b is None).  The backward takes the gradients of
    both outputs, recomputes everything from w and alpha and writes their sum at alpha; w gets no gradient (floor has none:
    the composition accumulates a tensor of zeros in weight.grad, this route leaves it None).
    delta / zp: one fp32 value per row."""

    @staticmethod
    def forward(ctx, w, alpha, delta, zp, n_levels, gamma, zeta, reg_b):
        from . import hip
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(w, alpha, delta, zp)
        ctx.grid = (n_levels, gamma, zeta, reg_b)
        w_hat, reg = hip.adaround_fwd(w, alpha, delta, zp, n_levels, gamma, zeta, reg_b)
        if reg is None:
            reg = torch.empty((), dtype=torch.float32, device=w.device)
            ctx.mark_non_differentiable(reg)
        return w_hat, reg

    @staticmethod
    def backward(ctx, gw, greg):
        from . import hip
        w, alpha, delta, zp = ctx.saved_tensors
        n_levels, gamma, zeta, reg_b = ctx.grid
        if gw is None:
            gw = torch.zeros_like(alpha)
        if gw.dtype != torch.float32 or hip.adaround_rows(gw) is None:
            gw = gw.float().contiguous()                   # (a split layer's halves, channel slices of the torch.cat gradient, are read in place)
        if reg_b is None or greg is None:
            reg_b = greg = None
        else:
            greg = greg.reshape(1).float()
        galpha = hip.adaround_bwd(gw, w, alpha, delta, zp, n_levels, gamma, zeta, reg_b, greg)
        return None, galpha, None, None, None, None, None, None


class AdaRoundQuantizer(nn.Module):
    # see UniformAffineQuantizer._STATE_ATTRS (resume_cali_model re-attaches delta / zero_point as plain tensors, reference
    # utils.py:409-417: QuantModel's packed weights, HIP graphs and prepared contexts must notice)
    _STATE_ATTRS = frozenset(("alpha", "delta", "zero_point", "soft_targets", "round_mode", "n_bits", "n_levels", "sym"))

    def __setattr__(self, name, value):
        if name in self._STATE_ATTRS:
            from . import engine
            engine.bump_state()
        super().__setattr__(name, value)

    def __delattr__(self, name):
        if name in self._STATE_ATTRS:
            from . import engine
            engine.bump_state()
        super().__delattr__(name)

    def __init__(self, uaq: UniformAffineQuantizer, weight_tensor: torch.Tensor, round_mode='learned_round_sigmoid'):
        super().__init__()
        # inherit the uniform quantiser's grid
        self.n_bits = uaq.n_bits
        self.sym = uaq.sym
        self.delta = uaq.delta
        self.zero_point = uaq.zero_point
        self.n_levels = uaq.n_levels
        self.round_mode = round_mode
        self.alpha = None
        self.soft_targets = False
        # rectified-sigmoid stretch parameters
        self.gamma, self.zeta = -0.1, 1.1
        self.beta = 2 / 3
        self.init_alpha(x=weight_tensor.clone())

    def rounding(self, x):
        """Integer (pre-zero-point) codes for the active rounding mode."""
        scaled = x / self.delta
        if self.round_mode == 'nearest':
            return torch.round(scaled)
        if self.round_mode == 'nearest_ste':
            return round_ste(scaled)
        if self.round_mode == 'stochastic':
            base = torch.floor(scaled)
            logger.info('Draw stochastic sample')
            return base + torch.bernoulli(scaled - base)
        if self.round_mode == 'learned_hard_sigmoid':
            base = torch.floor(scaled)
            up = self.get_soft_targets() if self.soft_targets else (self.alpha >= 0).float()
            return base + up
        raise ValueError('Wrong rounding mode')

    def _per_row(self, name, x):
        """self.<name> (delta / zero_point) as one fp32 value per row of `x` on its device, or None when the composition would
        not broadcast it that way: a per-row fp32 tensor of x's rank with every trailing dimension 1 is viewed; an fp32 scalar
        tensor or a Python number is expanded once and kept until the attribute or its contents change."""
        v, rows = getattr(self, name), x.shape[0]
        if torch.is_tensor(v):
            if v.dtype != torch.float32 or v.device != x.device or v.requires_grad:
                return None
            if v.dim() == x.dim() and tuple(v.shape) == (rows,) + (1,) * (x.dim() - 1):
                return v.reshape(rows)
            if v.numel() != 1:
                return None
            key = (id(v), v._version, rows)
        elif isinstance(v, (int, float)):
            key = (float(v), rows, x.device)
        else:
            return None
        kept = self.__dict__.setdefault('_row_cache', {})
        if name not in kept or kept[name][0] != key:
            full = torch.full((rows,), float(v), dtype=torch.float32, device=x.device) if not torch.is_tensor(v) \
                else v.reshape(1).expand(rows).contiguous()
            kept[name] = (key, full, v)                    # (v is kept so that its id stays its own)
        return kept[name][1]

    def _fused_args(self, x):
        """(delta, zero_point) rows for FusedAdaRound when this call takes the fused route (engine.FUSED_ADAROUND, DESIGN.md
        §4.20), else None: the composition below runs unchanged."""
        from . import engine, hip
        a = self.alpha
        if not (engine.FUSED_ADAROUND and self.round_mode == 'learned_hard_sigmoid' and self.soft_targets
                and torch.is_grad_enabled() and torch.is_tensor(a) and a.requires_grad):
            return None
        if not (x.dtype == torch.float32 and a.dtype == torch.float32 and x.device == a.device and engine.adaround_device_ok(x)
                and x.dim() >= 1 and a.shape == x.shape and a.is_contiguous() and a.data_ptr() % 16 == 0
                and 0 < x.numel() < 2 ** 31 and hip.adaround_rows(x) is not None):
            return None
        delta, zp = self._per_row('delta', x), self._per_row('zero_point', x)
        return None if delta is None or zp is None else (delta, zp)

    def forward(self, x):
        fused = self._fused_args(x)
        if fused is not None:
            b = self.__dict__.get('_reg_b')                # the exponent ReconstructionObjective.arm() announced, or None
            w_hat, reg = FusedAdaRound.apply(x.detach(), self.alpha, fused[0], fused[1], self.n_levels, self.gamma, self.zeta, b)
            if b is not None:
                self.__dict__['_reg_sum'] = (b, reg)
            return w_hat
        codes = torch.clamp(self.rounding(x) + self.zero_point, 0, self.n_levels - 1)
        return (codes - self.zero_point) * self.delta

    def get_soft_targets(self):
        return torch.clamp(torch.sigmoid(self.alpha) * (self.zeta - self.gamma) + self.gamma, 0, 1)

    def init_alpha(self, x: torch.Tensor):
        """alpha such that the rectified sigmoid equals the fractional part of w/delta
        (reference adaptive_rounding.py:66-74)."""
        if self.round_mode != 'learned_hard_sigmoid':
            raise NotImplementedError
        scaled = x / self.delta
        rest = scaled - torch.floor(scaled)
        self.alpha = nn.Parameter(-torch.log((self.zeta - self.gamma) / (rest - self.gamma) - 1))

    def extra_repr(self):
        return f'bit={self.n_bits}, symmetric={self.sym}, round_mode={self.round_mode}'
