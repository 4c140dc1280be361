"""Quantisers and the quantised Conv/Linear wrapper — MI355X-native counterpart of the reference's
qdiff/quant_layer.py (same public names, constructor signatures, attributes and state-dict keys).

What differs from the reference: with weight *and* activation quantisation switched on,
`QuantModule.forward` does not simulate integers in fp32 (reference quant_layer.py:256-276); it
quantises the input once to int8 (K1), and runs the contraction on MFMA-int8 with int4/int8 packed
weights and a fused dequantising epilogue (K3/K4, csrc/igemm_i8.hip).  The weight codes are packed
once per quantiser state (the reference re-quantises every weight tensor on every forward).

The fp32 simulation itself (`UniformAffineQuantizer.forward`) is kept as a differentiable torch
function because calibration code and the scripts call quantisers directly; it is not used by the
(True, True) inference path.
"""
import logging
import warnings
from typing import Union

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import engine, hip

logger = logging.getLogger(__name__)


class StraightThrough(nn.Module):
    """Identity placeholder (reference quant_layer.py:11-16)."""

    def __init__(self, channel_num: int = 1):
        super().__init__()

    def forward(self, input):
        return input


def round_ste(x: torch.Tensor):
    """Round with a straight-through gradient (reference quant_layer.py:19-23)."""
    return x + (x.round() - x).detach()


def lp_loss(pred, tgt, p=2.0, reduction='none'):
    """L_p reconstruction loss (reference quant_layer.py:26-33)."""
    err = (pred - tgt).abs().pow(p)
    return err.sum(1).mean() if reduction == 'none' else err.mean()


class FusedFakeQuant(torch.autograd.Function):
    """y = (clamp(round_ste(x / delta) + zp, lo, hi) - zp) * delta as ONE HIP launch forward and ONE backward
    (csrc/fakequant.hip) instead of the ~18 elementwise kernels autograd runs for the composition — the activation phase
    of calibration differentiates this expression for every quantised activation of a unit, every iteration
    (reference block_recon.py:72-110, quant_layer.py:82-88).  Same arithmetic operation by operation: y and dL/dx are
    bit-identical to the composition, dL/d(delta) differs by summation order only."""

    @staticmethod
    def forward(ctx, x, delta, zp, lo, hi):
        from . import hip
        xc = x.contiguous()
        if xc.data_ptr() % 16:                             # a contiguous VIEW at an odd offset: the kernels use 16-byte accesses
            xc = xc.clone()
        ctx.save_for_backward(xc, delta, zp)
        ctx.grid = (lo, hi)
        return hip.fakequant_fwd(xc, delta, zp, lo, hi).view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        from . import hip
        x, delta, zp = ctx.saved_tensors
        gy = gy.contiguous()
        if gy.data_ptr() % 16:
            gy = gy.clone()
        gx, gd = hip.fakequant_bwd(x, gy, delta, zp, *ctx.grid)
        return gx.view(gy.shape), gd.reshape(delta.shape), None, None, None


FUSED_FAKEQUANT = os.environ.get("QDIFF_FUSED_FAKEQUANT", "1") != "0"
# channel-wise 'mse' initialisation: vectorised over channels on the GPU; on the host the reference's per-channel loop
# (bit-faithful to its CPU results) unless this is set
VECTORISED_MSE_INIT = os.environ.get("QDIFF_VECTORISED_MSE_INIT", "0") == "1"


class UniformAffineQuantizer(nn.Module):
    """Uniform affine (asymmetric) / symmetric quantiser.

    Constructor keywords, attributes (`delta`, `zero_point`, `inited`, `sym`, `n_bits`, `n_levels`,
    `running_stat`, `leaf_param`, `x_min`, `x_max`) and the lazy data-dependent initialisation on the
    first tensor seen follow reference quant_layer.py:36-200.
    """

    # attributes whose (re-)assignment changes what the integer path bakes into device tensors — or takes the layer off that
    # path (data-dependent initialisation, range tracking): QuantModel re-validates its cached "whole model on the integer
    # path, these plans" verdict — and with it its HIP graphs and prepared contexts — when engine.STATE_GENERATION has moved
    _STATE_ATTRS = frozenset(("inited", "running_stat", "delta", "zero_point", "n_bits", "n_levels", "sym", "always_zero"))

    def __setattr__(self, name, value):
        if name in self._STATE_ATTRS:
            engine.bump_state()
        super().__setattr__(name, value)

    def __delattr__(self, name):
        if name in self._STATE_ATTRS:
            engine.bump_state()
        super().__delattr__(name)

    def __init__(self, n_bits: int = 8, symmetric: bool = False, channel_wise: bool = False,
                 scale_method: str = 'max', leaf_param: bool = False, always_zero: bool = False):
        super().__init__()
        self.sym = symmetric
        self.n_bits = n_bits
        self.n_levels = 2 ** n_bits if not symmetric else 2 ** (n_bits - 1) - 1
        self.delta = None
        self.zero_point = None
        self.inited = False
        self.leaf_param = leaf_param
        self.channel_wise = channel_wise
        self.scale_method = scale_method
        self.running_stat = False
        self.always_zero = always_zero
        if leaf_param:
            self.x_min, self.x_max = None, None

    # -- integer grid -------------------------------------------------------------------------
    def code_range(self):
        """[lo, hi] of the integer codes (reference quant_layer.py:84-87)."""
        if self.sym:
            return -self.n_levels - 1, self.n_levels
        return 0, self.n_levels - 1

    # -- initialisation -----------------------------------------------------------------------
    def ensure_init(self, x: torch.Tensor):
        """Data-dependent init from the first tensor seen (reference quant_layer.py:68-75)."""
        if self.inited:
            return
        if x.dtype != torch.float32:
            x = x.float()                                  # an fp16 activation stream: ranges and step sizes are fp32 all the same
        delta, zero_point = self.init_quantization_scale(x, self.channel_wise)
        self.delta = nn.Parameter(delta) if self.leaf_param else delta
        self.zero_point = zero_point
        self.inited = True

    def forward(self, x: torch.Tensor):
        self.ensure_init(x)
        if self.running_stat:
            self.act_momentum_update(x)
        lo, hi = self.code_range()
        if (FUSED_FAKEQUANT and x.is_cuda and torch.is_grad_enabled() and x.dtype == torch.float32 and torch.is_tensor(self.delta)
                and self.delta.numel() == 1 and self.delta.dtype == torch.float32 and (x.requires_grad or self.delta.requires_grad)):
            # calibration on the GPU (autograd through the quantiser): fused forward / backward kernels
            zp = self.zero_point
            zp = zp.detach().reshape(1).float() if torch.is_tensor(zp) else torch.full((1,), float(zp), device=x.device)
            return FusedFakeQuant.apply(x, self.delta, zp, lo, hi)
        codes = torch.clamp(round_ste(x / self.delta) + self.zero_point, lo, hi)
        return (codes - self.zero_point) * self.delta

    def act_momentum_update(self, x: torch.Tensor, act_range_momentum: float = 0.95):
        """EMA range tracking used during calibration (reference quant_layer.py:91-110)."""
        assert self.inited and self.leaf_param
        m = act_range_momentum
        self.x_min = self.x_min * m + x.data.min() * (1 - m)
        self.x_max = self.x_max * m + x.data.max() * (1 - m)
        if self.sym:
            delta = torch.max(self.x_min.abs(), self.x_max.abs()) / self.n_levels
        elif self.always_zero:
            delta = self.x_max / (self.n_levels - 1)
        else:
            delta = (self.x_max - self.x_min) / (self.n_levels - 1)
        delta = torch.clamp(delta, min=1e-8)
        if not self.sym:
            self.zero_point = 0 if self.always_zero else (-self.x_min / delta).round()
        self.delta = nn.Parameter(delta)

    def _init_max_channelwise(self, x):
        """Vectorised form of the reference's per-channel Python loop (quant_layer.py:114-136,
        142-160).  fp64 arithmetic reproduces the reference's Python-float math exactly: delta is
        a double quotient rounded to fp32, zero_point is round-half-even of a double quotient."""
        flat = x.detach().reshape(x.shape[0], -1).double()
        mx, mn = flat.max(dim=1)[0], flat.min(dim=1)[0]
        lo = torch.clamp(mn, max=0.0)
        hi = torch.clamp(mx, min=0.0)
        if 'scale' in self.scale_method:
            lo = lo * (self.n_bits + 2) / 8
            hi = hi * (self.n_bits + 2) / 8
        if self.sym:
            delta = torch.maximum(lo.abs(), hi) / self.n_levels
        else:
            delta = (mx - mn) / (self.n_levels - 1)
        if bool((delta < 1e-8).any()):
            warnings.warn('Quantization range close to zero in at least one channel')
            delta = torch.clamp(delta, min=1e-8)
        if self.sym or self.always_zero:
            zp = torch.zeros_like(delta)
        else:
            zp = torch.round(-lo / delta)
        shape = (-1,) + (1,) * (x.dim() - 1)
        return delta.to(x.dtype).view(shape), zp.to(x.dtype).view(shape)

    def _init_mse_channelwise(self, x):
        """All channels of the reference's per-channel LAPQ range search (quant_layer.py:138-140,162-177) at once: for each
        of the 80 shrink factors one quantise + L_2.4 score over the whole tensor with per-channel (delta, zero_point), then
        a per-channel arg-min with the loop's first-strictly-better rule.  The reference loops over output channels in
        Python (80 x ~12 kernels per channel: hours for the 100k channels of SD); same operations per element here, the
        per-channel mean is a row reduction instead of a whole-tensor one (scores agree to fp32 summation order, so a
        channel whose two best candidates tie to ~1e-7 may pick the neighbouring factor)."""
        flat = x.detach().reshape(x.shape[0], -1)
        x_max, x_min = flat.max(dim=1, keepdim=True)[0], flat.min(dim=1, keepdim=True)[0]
        levels = 2 ** self.n_bits - 1
        best = torch.full_like(x_max, 1e+10)
        delta, zero_point = torch.zeros_like(x_max), torch.zeros_like(x_max)
        for i in range(80):
            new_max = x_max * (1.0 - (i * 0.01))
            new_min = x_min * (1.0 - (i * 0.01))
            d = (new_max / levels) if self.always_zero else ((new_max - new_min) / levels)
            z = torch.zeros_like(d) if self.always_zero else (-new_min / d).round()
            xq = (torch.clamp(torch.round(flat / d) + z, 0, self.n_levels - 1) - z) * d
            score = (flat - xq).abs().pow(2.4).mean(dim=1, keepdim=True)
            better = score < best
            best = torch.where(better, score, best)
            delta = torch.where(better, d, delta)
            zero_point = torch.where(better, z, zero_point)
        shape = (-1,) + (1,) * (x.dim() - 1)
        return delta.view(shape), zero_point.view(shape)

    def _init_mse_fused(self, x, channel_wise):
        """The 'mse' range search as ONE qd_mse_search call (engine.FUSED_MSE_INIT; csrc/mse_search.hip): None
        when the route does not apply — the knob, the method, fp32 on a device the kernel runs on, rows consecutive in memory
        (a dense tensor, a weight[:, a:b] slice, an activation's channel slice as B rows), fewer than 2^31 elements — or when
        the whole-tensor search took no candidate: the caller's composition then returns what it always returned."""
        if not (engine.FUSED_MSE_INIT and self.scale_method == 'mse' and torch.is_tensor(x) and x.dtype == torch.float32
                and engine.mse_init_device_ok(x)):
            return None
        xd = x.detach()
        geo = hip.adaround_rows(xd)
        if geo is None or geo[0] * geo[1] >= 2 ** 31:
            return None
        delta, zero_point, x_min, x_max, index, _ = hip.mse_search(xd, channel_wise, self.n_bits, self.n_levels, self.always_zero)
        if channel_wise:                                   # a row where nothing was taken holds (0, 0), as the composition's
            shape = (-1,) + (1,) * (x.dim() - 1)
            return delta.view(shape), zero_point.view(shape)
        if int(index) < 0:
            return None
        if self.leaf_param:
            self.x_min, self.x_max = x_min.reshape(()), x_max.reshape(())
        return delta.reshape(()), (0 if self.always_zero else zero_point.reshape(()))

    def init_quantization_scale(self, x: torch.Tensor, channel_wise: bool = False, _fused: bool = True):
        fused = self._init_mse_fused(x, channel_wise) if _fused else None
        if fused is not None:
            return fused
        if channel_wise:
            if 'max' in self.scale_method:
                return self._init_max_channelwise(x)
            if self.scale_method == 'mse' and (x.is_cuda or VECTORISED_MSE_INIT):
                return self._init_mse_channelwise(x)
            xc = x.clone().detach()
            delta = torch.zeros(xc.shape[0], dtype=x.dtype, device=x.device)
            zero_point = torch.zeros_like(delta)
            for c in range(xc.shape[0]):               # (a channel-wise tensor the fused search refused stays on the composition)
                delta[c], zero_point[c] = self.init_quantization_scale(xc[c], channel_wise=False, _fused=False)
            shape = (-1,) + (1,) * (x.dim() - 1)
            return delta.view(shape), zero_point.view(shape)

        if self.leaf_param:
            self.x_min = x.data.min()
            self.x_max = x.data.max()
        if 'max' in self.scale_method:
            raw_min, raw_max = x.min().item(), x.max().item()
            x_min, x_max = min(raw_min, 0), max(raw_max, 0)
            if 'scale' in self.scale_method:
                x_min = x_min * (self.n_bits + 2) / 8
                x_max = x_max * (self.n_bits + 2) / 8
            if self.sym:
                delta = max(abs(x_min), x_max) / self.n_levels
            else:
                delta = float(raw_max - raw_min) / (self.n_levels - 1)
            if delta < 1e-8:
                warnings.warn('Quantization range close to zero: [{}, {}]'.format(x_min, x_max))
                delta = 1e-8
            zero_point = 0 if (self.sym or self.always_zero) else round(-x_min / delta)
            return torch.tensor(delta).type_as(x), zero_point
        if self.scale_method == 'mse':
            # LAPQ-style range search (reference quant_layer.py:162-177)
            x_max, x_min = x.max(), x.min()
            best_score, delta, zero_point = 1e+10, None, None
            for i in range(80):
                new_max = x_max * (1.0 - (i * 0.01))
                new_min = x_min * (1.0 - (i * 0.01))
                score = lp_loss(x, self.quantize(x, new_max, new_min), p=2.4, reduction='all')
                if score < best_score:
                    best_score = score
                    span = new_max if self.always_zero else (new_max - new_min)
                    delta = span / (2 ** self.n_bits - 1)
                    zero_point = 0 if self.always_zero else (-new_min / delta).round()
            return delta, zero_point
        raise NotImplementedError(self.scale_method)

    def quantize(self, x, max, min):
        span = max if self.always_zero else (max - min)
        delta = span / (2 ** self.n_bits - 1)
        zero_point = 0 if self.always_zero else (-min / delta).round()
        codes = torch.clamp(torch.round(x / delta) + zero_point, 0, self.n_levels - 1)
        return (codes - zero_point) * delta

    def bitwidth_refactor(self, refactored_bit: int):
        self.n_bits = refactored_bit
        self.n_levels = 2 ** self.n_bits

    def extra_repr(self):
        return (f'bit={self.n_bits}, scale_method={self.scale_method}, symmetric={self.sym}, '
                f'channel_wise={self.channel_wise}, leaf_param={self.leaf_param}')


def _module_kind(m):
    if isinstance(m, nn.Conv2d):
        return 'conv2d'
    if isinstance(m, nn.Conv1d):
        return 'conv1d'
    if isinstance(m, nn.Linear):
        return 'linear'
    raise TypeError(f'QuantModule wraps Conv2d / Conv1d / Linear, got {type(m).__name__}')


class QuantModule(nn.Module):
    """Quantised Conv2d / Conv1d / Linear.  Public surface as reference quant_layer.py:203-294:
    attributes `weight`, `bias`, `org_weight`, `org_bias`, `use_weight_quant`, `use_act_quant`,
    `weight_quantizer[_0]`, `act_quantizer[_0]`, `split`, `ignore_reconstruction`,
    `activation_function`, `fwd_kwargs`, `fwd_func`, `disable_act_quant`; `forward(input, split=0)`.
    """

    def __init__(self, org_module: Union[nn.Conv2d, nn.Linear, nn.Conv1d], weight_quant_params: dict = {},
                 act_quant_params: dict = {}, disable_act_quant: bool = False, act_quant_mode: str = 'qdiff'):
        super().__init__()
        self.weight_quant_params = weight_quant_params
        self.act_quant_params = act_quant_params
        self.kind = _module_kind(org_module)
        if self.kind == 'linear':
            self.fwd_kwargs = dict()
            self.fwd_func = F.linear
        else:
            self.fwd_kwargs = dict(stride=org_module.stride, padding=org_module.padding,
                                   dilation=org_module.dilation, groups=org_module.groups)
            self.fwd_func = F.conv2d if self.kind == 'conv2d' else F.conv1d
        self.weight = org_module.weight
        self.org_weight = org_module.weight.data.clone()      # plain attribute, as in the reference
        if org_module.bias is not None:
            self.bias = org_module.bias
            self.org_bias = org_module.bias.data.clone()
        else:
            self.bias = None
            self.org_bias = None
        self.use_weight_quant = False
        self.use_act_quant = False
        self.act_quant_mode = act_quant_mode
        self.disable_act_quant = disable_act_quant
        self.weight_quantizer = UniformAffineQuantizer(**self.weight_quant_params)
        if self.act_quant_mode == 'qdiff':
            self.act_quantizer = UniformAffineQuantizer(**self.act_quant_params)
        self.split = 0
        self.activation_function = StraightThrough()
        self.ignore_reconstruction = False
        self.extra_repr = org_module.extra_repr
        # frozen integer state (not part of the state dict)
        self._pack, self._pack_key = None, None
        self._plan, self._plan_key = None, None
        self._wdq, self._wdq_key = None, None

    # see UniformAffineQuantizer._STATE_ATTRS: re-assigned weights / quantiser objects / switches invalidate QuantModel's verdict
    _STATE_ATTRS = frozenset(("weight", "bias", "split", "disable_act_quant", "act_quant_mode", "use_weight_quant", "use_act_quant",
                              "weight_quantizer", "weight_quantizer_0", "act_quantizer", "act_quantizer_0"))

    def __setattr__(self, name, value):
        if name in self._STATE_ATTRS:
            engine.bump_state()
        super().__setattr__(name, value)

    def __delattr__(self, name):
        if name in self._STATE_ATTRS:
            engine.bump_state()
        super().__delattr__(name)

    # -- reference-visible controls -----------------------------------------------------------
    def set_quant_state(self, weight_quant: bool = False, act_quant: bool = False):
        self.use_weight_quant = weight_quant
        self.use_act_quant = act_quant

    def set_split(self):
        self.weight_quantizer_0 = UniformAffineQuantizer(**self.weight_quant_params)
        if self.act_quant_mode == 'qdiff':
            self.act_quantizer_0 = UniformAffineQuantizer(**self.act_quant_params)

    def set_running_stat(self, running_stat: bool):
        engine.bump_state()
        if self.act_quant_mode == 'qdiff':
            self.act_quantizer.running_stat = running_stat
            if self.split != 0:
                self.act_quantizer_0.running_stat = running_stat

    def _note_split(self, split):
        """Sticky split bookkeeping (reference quant_layer.py:249-254)."""
        if split != 0 and self.split != 0:
            assert split == self.split
        elif split != 0:
            logger.info(f"split at {split}!")
            self.split = split
            self.set_split()

    # -- helpers ------------------------------------------------------------------------------
    def _weight_quantizers(self):
        return [self.weight_quantizer] if self.split == 0 else [self.weight_quantizer, self.weight_quantizer_0]

    def _act_quantizers(self):
        return [self.act_quantizer] if self.split == 0 else [self.act_quantizer, self.act_quantizer_0]

    def _weight_slices(self):
        if self.split == 0:
            return [self.weight]
        return [self.weight[:, :self.split, ...], self.weight[:, self.split:, ...]]

    def _input_slices(self, x):
        if self.split == 0:
            return [x]
        return [x[:, :self.split], x[:, self.split:]]

    def _geometry(self):
        """(kh, kw, stride, pad) or None when the integer kernel does not cover the configuration."""
        if self.kind == 'linear':
            return 1, 1, 1, 0
        kw = self.fwd_kwargs
        one = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * (2 if self.kind == 'conv2d' else 1)
        st, pd, dl = one(kw['stride']), one(kw['padding']), one(kw['dilation'])
        if kw['groups'] != 1 or any(d != 1 for d in dl) or len(set(st)) != 1 or len(set(pd)) != 1:
            return None
        ks = self.__dict__.get('_ksize')                 # remembered: the fp32 weight may have been released (load_packed)
        if ks is None:
            ks = self.__dict__['_ksize'] = tuple(self.weight.shape[2:])
        if self.kind == 'conv1d':
            return 1, ks[0], st[0], pd[0]
        return ks[0], ks[1], st[0], pd[0]

    def int_ready(self):
        """True when this module will take the integer path on its next forward.  A (True, True) module whose
        configuration the integer kernels do not cover (groups, dilation, unequal stride / padding) raises instead of
        silently running the fp32 simulation; `engine.SIMULATE = True` selects the simulation on purpose
        (bench.py times it on the GPU as the reference fake-quant denominator)."""
        if not (self.use_weight_quant and self.use_act_quant and not self.disable_act_quant
                and self.act_quant_mode == 'qdiff') or engine.SIMULATE:
            return False
        if self._geometry() is None:
            raise hip.HipEngineError(
                f"QuantModule({self.kind}, {self.fwd_kwargs}): grouped / dilated / anisotropic convolutions have no integer "
                "kernel; set qdiff.engine.SIMULATE = True to run the fp32 simulation explicitly")
        return True

    def dequantized_weight(self):
        """fp32 weight after fake quantisation, cached per quantiser state (weights-only mode)."""
        qs = self._weight_quantizers()
        key = (tuple(engine.quantizer_key(q) for q in qs), engine.tensor_version(self.weight), self.weight.data_ptr(), self.split)
        if self._wdq_key != key or torch.is_grad_enabled():
            parts = [q(w) for q, w in zip(qs, self._weight_slices())]
            w = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
            if torch.is_grad_enabled():
                return w
            self._wdq, self._wdq_key = w, key
        return self._wdq

    # -- integer plan -------------------------------------------------------------------------
    def invalidate(self):
        """Drop the packed weights / epilogue constants.  The caches below notice re-assigned
        quantiser attributes and in-place updates that bump a tensor's version counter
        (optimizer steps, load_state_dict, `p.mul_()` ...); writes through `.data` bypass version
        tracking, so call this (or QuantModel.invalidate_plans()) after such an edit."""
        engine.bump_state()
        self._pack_key = self._plan_key = self._wdq_key = None
        self.__dict__.pop('_wonly_cache', None)
        self.__dict__.pop('_wonly_geglu_cache', None)
        self.__dict__.pop('_geglu_cache', None)
        self.__dict__.pop('_heads_cache', None)
        self.__dict__.pop('_frozen_pack', None)
        self.__dict__.pop('_frozen_geglu_pack', None)

    def load_packed(self, pack, geglu_pack=None):
        """Install packed weights read from a packed checkpoint (utils.load_packed_ckpt): the integer path then never
        looks at the fp32 weight / AdaRound alpha again (they can be freed); invalidate() returns to the live weights."""
        self._geometry()                                   # records the kernel size while the weight still has its shape
        engine.bump_state()
        self.__dict__['_frozen_pack'] = pack
        self.__dict__['_frozen_geglu_pack'] = geglu_pack
        self._pack_key = self._plan_key = None
        self.__dict__.pop('_wonly_cache', None)
        self.__dict__.pop('_wonly_geglu_cache', None)
        self.__dict__.pop('_geglu_cache', None)
        self.__dict__.pop('_heads_cache', None)

    def plan_keys(self):
        """(wkey, akey): identity of everything the packed weights resp. the whole plan are made from — quantiser objects and
        their tensors (object, in-place version, storage), the weight, the bias, the split.  conv_plan() rebuilds when they
        move; QuantModel compares them model-wide to decide whether its HIP graphs / prepared contexts are still valid."""
        wqs, aqs = self._weight_quantizers(), self._act_quantizers()
        frozen = self.__dict__.get('_frozen_pack')
        if frozen is not None:
            wkey = ('frozen', id(frozen))
        else:
            for q, w in zip(wqs, self._weight_slices()):
                if hasattr(q, 'ensure_init'):
                    q.ensure_init(w)
            wkey = (tuple(engine.quantizer_key(q) for q in wqs), engine.tensor_version(self.weight), self.weight.data_ptr(), self.split)
        bias_key = None if self.bias is None else (engine.tensor_version(self.bias), self.bias.data_ptr())
        return wkey, (wkey, tuple(engine.quantizer_key(q) for q in aqs), bias_key)

    def state_tensors(self):
        """Every tensor whose in-place modification must invalidate what was built from this module (QuantModel sums their
        version counters per evaluation: cheaper than re-deriving plan_keys())."""
        out = [self.weight, self.bias]
        qs = self._weight_quantizers() + (self._act_quantizers() if self.act_quant_mode == 'qdiff' else [])
        for q in qs:
            out += [getattr(q, n, None) for n in ("delta", "zero_point", "alpha")]
        return [t for t in out if torch.is_tensor(t)]

    def conv_plan(self):
        """Packed weights + epilogue constants for the current quantiser state (lazy, cached)."""
        wqs, aqs = self._weight_quantizers(), self._act_quantizers()
        wkey, akey = self.plan_keys()
        frozen = self.__dict__.get('_frozen_pack')
        if frozen is not None and self._pack_key != wkey:
            self._pack, self._pack_key, self._plan_key = frozen, wkey, None
        if self._pack_key != wkey:
            self._pack = engine.pack_module_weights(self.weight, wqs, self.split)
            self._pack_key, self._plan_key = wkey, None
        if self._plan_key != akey:
            kh, kw, stride, pad = self._geometry()
            self._plan = engine.build_conv_plan(self._pack, aqs, kh, kw, stride, pad, self.bias)
            self._plan_key = akey
        return self._plan

    def _init_act_quantizers(self, x):
        for q, xs in zip(self._act_quantizers(), self._input_slices(x)):
            q.ensure_init(xs)
            if q.running_stat:
                q.act_momentum_update(xs)

    def _forward_int(self, x, out_slot=None):
        self._init_act_quantizers(x)
        plan = self.conv_plan()
        if self.kind == 'conv2d':
            B, C, H, W = x.shape
            sb, sc, sh, sw = x.stride()
            if sh != W * sw:
                x = x.contiguous(memory_format=torch.channels_last)
                sb, sc, sh, sw = x.stride()
            xq = engine.quantize_rows(x, plan, B, C, H * W, (sb, sc, sw))
            Ho, Wo = engine.conv_out_hw(H, W, plan)
            out = engine.conv_forward(plan, xq, B, H, W, Ho, Wo, gn_stats=True, slot=out_slot)   # most conv outputs feed a GroupNorm
            y = out.view(B, Ho, Wo, plan.Cout).permute(0, 3, 1, 2)
            if hasattr(out, "qd_gn_part"):
                y.qd_gn_part = out.qd_gn_part
            return y
        if self.kind == 'conv1d':
            B, C, T = x.shape
            sb, sc, st = x.stride()
            xq = engine.quantize_rows(x, plan, B, C, T, (sb, sc, st))
            To = (T + 2 * plan.pad - plan.kw) // plan.stride + 1
            out = engine.conv_forward(plan, xq, B, 1, T, 1, To)
            return out.view(B, To, plan.Cout).permute(0, 2, 1)
        lead, K = x.shape[:-1], x.shape[-1]
        rows = x.reshape(-1, K)
        if rows.stride(1) != 1:
            rows = rows.contiguous()
        M = rows.shape[0]
        xq = engine.quantize_rows(rows, plan, 1, K, M, (0, 1, rows.stride(0)))
        out = engine.conv_forward(plan, xq, 1, 1, M, 1, M)
        return out.view(*lead, plan.Cout)

    # -- weights-only kernel (engine.WEIGHT_ONLY_KERNEL) ---------------------------------------------
    def _wonly_state(self):
        """Weights quantised, activations not (state (True, False) or disable_act_quant), no autograd, no simulation, knob set."""
        return (engine.WEIGHT_ONLY_KERNEL is not None and not engine.SIMULATE and self.use_weight_quant
                and not (self.use_act_quant and not self.disable_act_quant and self.act_quant_mode == 'qdiff')
                and not torch.is_grad_enabled())

    def wonly_plan(self):
        """engine.WonlyPlan of the current weight quantisers for engine.WEIGHT_ONLY_KERNEL, or None when the kernel does not
        take this layer (grouped / dilated convolution, a weight quantiser the packer refuses — symmetric, per-tensor, AdaRound
        soft targets — or bf16 operands with |q - z| > 256): the layer then keeps the library path.  Built from the pack of
        the integer path (or a packed checkpoint's frozen pack) without touching the activation quantisers; cached under the
        weight part of plan_keys() and dropped by invalidate()."""
        dt = engine.WEIGHT_ONLY_KERNEL
        if dt is None:
            return None
        geo = self._geometry()
        cache = self.__dict__.setdefault('_wonly_cache', [None, None])
        if geo is None:
            cache[0], cache[1] = None, None
            return None
        wkey, akey = self.plan_keys()
        key = (wkey, akey[2], dt)
        if cache[0] == key:
            return cache[1]
        frozen = self.__dict__.get('_frozen_pack')
        pack = None
        if frozen is not None:
            pack = frozen
        elif self._pack_key == wkey:
            pack = self._pack
        else:
            try:
                pack = engine.pack_module_weights(self.weight, self._weight_quantizers(), self.split)
            except hip.HipEngineError:
                pack = None
            else:
                self._pack, self._pack_key, self._plan_key = pack, wkey, None
        kh, kw, stride, pad = geo
        plan = engine.build_wonly_plan(pack, kh, kw, stride, pad, self.bias, dt) if pack is not None else None
        cache[0], cache[1] = key, plan
        return plan

    def wonly_geglu_plan(self):
        """engine.WonlyPlan of a GEGLU projection over the (value tile, gate tile) interleaved pack, for the value * gelu(gate)
        epilogue of the weights-only contraction (engine.wonly_forward_geglu), or None: not a Linear, a split input, halves
        that are not whole 32-row tiles, a weight quantiser the packer refuses, bf16 operands with |q - z| > 256.  The pack is,
        in this order, the interleaved pack of a packed checkpoint, the layer's own (possibly frozen) pack gathered tile by tile
        — nothing is re-quantised, so freed fp32 weights are no obstacle — or a fresh pack of the permuted rows.  Like
        wonly_plan() it never touches the activation quantisers, is cached under the weight part of plan_keys() and the
        operand type, and is dropped by invalidate() / load_packed()."""
        dt = engine.WEIGHT_ONLY_KERNEL
        if dt is None or self.kind != 'linear' or self.split != 0:
            return None
        wkey, akey = self.plan_keys()
        key = (wkey, akey[2], dt)
        cache = self.__dict__.setdefault('_wonly_geglu_cache', [None, None])
        if cache[0] == key:
            return cache[1]
        plan = None
        base = self.wonly_plan()                             # the layer's own pack (frozen, the integer path's, or fresh)
        if base is not None and base.Cout % 64 == 0:
            F = base.Cout // 2
            pack = self.__dict__.get('_frozen_geglu_pack')
            if pack is None:
                pack = engine.pack_select_tiles(base.pack, engine.geglu_row_perm(F, base.pack.wq.device))
            if pack is None and not self._weights_freed():
                try:
                    pack = engine.pack_module_weights(self.weight, self._weight_quantizers(), 0,
                                                      row_perm=engine.geglu_row_perm(F, self.weight.device))
                except hip.HipEngineError:
                    pack = None
            if pack is not None:
                plan = engine.build_wonly_plan(pack, 1, 1, 1, 0, self.bias, dt, geglu=True)
        cache[0], cache[1] = key, plan
        return plan

    def wonly_ready(self):
        """True when the next forward of this module runs the weights-only kernel (kept apart from int_ready(): the blocks'
        fused integer routes must not engage in this state)."""
        return self._wonly_state() and self.wonly_plan() is not None

    def _weights_freed(self):
        return self.__dict__.get('_frozen_pack') is not None and self.weight.numel() == 0

    def _forward_wonly(self, x, plan):
        out_dtype, cast = engine.wonly_out_dtype(x.device.type)
        if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            x = x.float()
        if self.kind == 'conv2d':
            B, C, H, W = x.shape
            sb, sc, sh, sw = x.stride()
            if sh != W * sw:
                x = x.contiguous(memory_format=torch.channels_last)
                sb, sc, sh, sw = x.stride()
            xh = engine.wonly_rows(x, plan, B, C, H * W, (sb, sc, sw))
            Ho, Wo = engine.conv_out_hw(H, W, plan)
            y = engine.wonly_forward(plan, xh, B, H, W, Ho, Wo, out_dtype).view(B, Ho, Wo, plan.Cout).permute(0, 3, 1, 2)
        elif self.kind == 'conv1d':
            B, C, T = x.shape
            xh = engine.wonly_rows(x, plan, B, C, T, x.stride())
            To = (T + 2 * plan.pad - plan.kw) // plan.stride + 1
            y = engine.wonly_forward(plan, xh, B, 1, T, 1, To, out_dtype).view(B, To, plan.Cout).permute(0, 2, 1)
        else:
            lead, K = x.shape[:-1], x.shape[-1]
            rows = x.reshape(-1, K)
            if rows.stride(1) != 1:
                rows = rows.contiguous()
            M = rows.shape[0]
            xh = engine.wonly_rows(rows, plan, 1, K, M, (0, 1, rows.stride(0)))
            y = engine.wonly_forward(plan, xh, 1, 1, M, 1, M, out_dtype).view(*lead, plan.Cout)
        return y if cast is None else y.to(cast)

    def forward_rows(self, xh, B, H, W, Ho=None, Wo=None, rowbias=None, residual=None, out_dtype=torch.float32):
        """Weights-only path for a producer that already emitted this module's fp16 / bf16 operand rows (fused blocks; the
        counterpart of forward_codes).  xh: rows [B*H*W][plan.ldx]; rowbias: fp32 [B][Cout] added per sample; residual: rows
        [B*Ho*Wo][Cout] added in the epilogue.  Returns channels-last rows [B*Ho*Wo][Cout]."""
        plan = self.wonly_plan()
        if Ho is None:
            Ho, Wo = engine.conv_out_hw(H, W, plan)
        return engine.wonly_forward(plan, xh, B, H, W, Ho, Wo, out_dtype, residual=residual, rowbias=rowbias)

    def geglu_plan(self):
        """Second plan of a GEGLU projection: rows packed (value tile, gate tile) interleaved for the fused
        value*gelu(gate)->quantise epilogue (engine.conv_forward_geglu).  None if the layer does not
        qualify (needs tile-ordered int4 weights and an even split into 32-row tiles)."""
        fz = self.__dict__.get('_frozen_geglu_pack')
        if self.__dict__.get('_frozen_pack') is not None:
            if fz is None:
                return None
            key = ('frozen', id(fz), engine.quantizer_key(self.act_quantizer))
            cache = self.__dict__.setdefault('_geglu_cache', [None, None])
            if cache[0] != key:
                cache[0], cache[1] = key, engine.build_conv_plan(fz, [self.act_quantizer], 1, 1, 1, 0, self.bias)
            return cache[1]
        F = self.weight.shape[0] // 2
        if self.kind != 'linear' or self.split != 0 or F % 32 != 0:
            return None
        wq, aq = self.weight_quantizer, self.act_quantizer
        if hasattr(wq, 'ensure_init'):
            wq.ensure_init(self.weight)
        key = (engine.quantizer_key(wq), engine.quantizer_key(aq), engine.tensor_version(self.weight), self.weight.data_ptr(),
               None if self.bias is None else (engine.tensor_version(self.bias), self.bias.data_ptr()))
        cache = self.__dict__.setdefault('_geglu_cache', [None, None])
        if cache[0] != key:
            pack = engine.pack_module_weights(self.weight, [wq], 0, row_perm=engine.geglu_row_perm(F, self.weight.device))
            cache[1] = engine.build_conv_plan(pack, [aq], 1, 1, 1, 0, self.bias) if (pack.tiled and pack.wbits == 4) else None
            cache[0] = key
        return cache[1]

    def head_plans(self, heads):
        """Three plans (q, k, v) of a fused qkv 1x1 projection whose output channels are ordered [head][q | k | v][d] (the
        QKVAttentionLegacy layout of the LDM AttentionBlock, reference quant_block.py:163-187 / openaimodel.py qkv conv1d):
        the rows of each role gathered head-major, so that each role runs as its own GEMM with the attention-operand
        epilogue (engine.project_heads) — per-output-channel weight quantisers make the row subsets exact.  With heads of
        a multiple of 32 channels the three operands are gathered tile by tile from the layer's own pack (also the frozen
        one of a packed checkpoint); otherwise the rows are packed again from the live weight.  None when the layer does
        not qualify (split input, a kernel wider than one tap, channels not divisible, frozen weights with ragged heads)."""
        if self.split != 0 or self.kind not in ('conv1d', 'linear'):
            return None
        pack = self.conv_plan().pack
        C3 = pack.Cout
        if C3 % (3 * heads) != 0 or pack.taps != 1 or not pack.tiled:
            return None
        d = C3 // (3 * heads)
        frozen = self.__dict__.get('_frozen_pack') is not None
        if frozen and d % 32 != 0:
            return None
        wkey, akey = self.plan_keys()
        key = (heads, akey)
        cache = self.__dict__.setdefault('_heads_cache', [None, None])
        if cache[0] != key:
            dev = pack.wq.device
            base = (torch.arange(heads, device=dev) * (3 * d))[:, None] + torch.arange(d, device=dev)[None, :]
            plans = []
            for role in range(3):
                rows = (base + role * d).reshape(-1)
                sub = engine.pack_select_tiles(pack, rows) if d % 32 == 0 else None
                if sub is None and not frozen:
                    sub = engine.pack_module_weights(self.weight, [self.weight_quantizer], 0, row_perm=rows)
                plans.append(None if sub is None else engine.build_conv_plan(sub, [self.act_quantizer], 1, 1, 1, 0, self.bias))
            cache[0], cache[1] = key, (plans if all(p is not None and p.pack.tiled for p in plans) else None)
        return cache[1]

    def forward_codes(self, xq, B, H, W, Ho=None, Wo=None, rowbias=None, residual=None, pad_tl=None, gn_stats=False, slot=None,
                      upsample2x=False):
        """Integer path for a producer that already emitted this module's int8 rows (fused blocks).
        slot: engine.CatSlot side that receives the output (a planned skip concatenation), see engine.conv_forward."""
        return engine.conv_forward(self.conv_plan(), xq, B, H, W, Ho, Wo, rowbias=rowbias, residual=residual,
                                   pad_tl=pad_tl, gn_stats=gn_stats, slot=slot, upsample2x=upsample2x)

    # -- forward ------------------------------------------------------------------------------
    qd_takes_out_slot = True

    def forward(self, input: torch.Tensor, split: int = 0, out_slot=None):
        """out_slot (engine-internal, optional): destination of the output inside a planned skip-concatenation buffer
        (engine.CatSlot); honoured on the integer conv2d path only, ignored (plain allocation) everywhere else."""
        self._note_split(split)
        if not torch.is_grad_enabled() and self.int_ready():
            return self.activation_function(self._forward_int(input, out_slot))
        if self._wonly_state() and engine.wonly_device_ok(input):
            plan = self.wonly_plan()
            if plan is not None:
                return self.activation_function(self._forward_wonly(input, plan))
        # simulated / floating-point states: (False, *), weights-only, or calibration under autograd
        if self._weights_freed():
            raise hip.HipEngineError(
                f"QuantModule({self.kind}): the fp32 weights were released by load_packed_ckpt(free_weights=True), so only the "
                "packed kernels can run it: the integer state (True, True), or the weights-only state with the weights-only "
                "kernel on (qdiff.engine.set_weight_only_kernel(torch.float16 | torch.bfloat16) or QDIFF_WEIGHT_ONLY=fp16|bf16)")
        if not self.disable_act_quant and self.use_act_quant and self.act_quant_mode == 'qdiff':
            parts = [q(xs) for q, xs in zip(self._act_quantizers(), self._input_slices(input))]
            input = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        if self.use_weight_quant:
            weight, bias = self.dequantized_weight(), self.bias
        else:
            weight, bias = self.org_weight, self.org_bias
        return self.activation_function(self.fwd_func(input, weight, bias, **self.fwd_kwargs))
