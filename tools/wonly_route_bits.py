#!/usr/bin/env python3
"""Host-side record of the block routes, for refactors that must not change them (CPU, on the emulators of tests/).

    python tools/wonly_route_bits.py record OUT.json          one tree: every model x knob combination below
    python tools/wonly_route_bits.py record --gpu OUT.json    one tree on the real library (cuda:0): counters and output hashes only
    python tools/wonly_route_bits.py compare A.json B.json    two records -> one two-column line per case, 'equal' or not

Per case it keeps the call list of the emulated entry points of qdiff.hip (names; for the producers, qd_rows_to_h16 and the
contraction also every shape argument and leading dimension), the engine.WONLY_FUSED / WONLY_GEGLU_EPI / WONLY_TEMB /
ATTN_H16_LAUNCHES counters and a SHA-256 of the output bytes.
Weights-only state, LDM family: fusion / wide / modulated-resampling / fp16 attention, each on and off; wide and modulated
without the fusion knob are kept (the host tests hold them to "changes nothing"), wide together with modulated only under fusion,
and every knob together with the one-launch embedding Linears.  DDIM family: under fusion, the DDIM knob, the embedding knob and
the fp16 attention each on and off.
Integer state (True, True), on tests/abi_emulator.py: every tiny model, churches_full, cifar_full and ldm_full, the call list
being the names of the emulated entry points and, for conv2d_i8 / conv2d_i8_group, the fields of each ConvCall; sd_tiny also as
a marked guidance pair (tests/cfg_pair_emulator.py).
--gpu installs no emulator: the tiny models in the states (True, True) and (True, False), with the fp16 layer kernel alone and
with every weights-only knob on (split-K and graph replay stay off: no floating-point reduction order is in play; with the layer
kernel off the state (True, False) is the torch library composition, whose bytes differ from one evaluation to the next)."""
import hashlib
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "q-diffusion_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

MODELS = ("ldm_tiny", "ldm_updown_tiny", "sd_tiny", "churches_full")
DDIM_MODELS = ("cifar_tiny", "cifar_full")
TINY = ("cifar_tiny", "ldm_tiny", "ldm_updown_tiny", "sd_tiny")
INT_FULL = ("churches_full", "cifar_full", "ldm_full")       # (the last two: self-attention on maps of T % 128 == 0 tokens)
# (fuse, wide, mod, temb)
KNOBS = ((0, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 1, 1, 0), (1, 1, 1, 1))
# (fuse, ddim, temb)
DDIM_KNOBS = ((1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1))
SHAPED = ("rows_to_h16", "conv2d_wq_h16", "layernorm_h16", "geglu_h16", "groupnorm_h16", "groupnorm_mod_h16",
          "groupnorm_resample_h16", "attn_h16", "temb_mlp_wq_h16")
INT_ENTRIES = ("quantize_act", "conv2d_i8", "conv2d_i8_group", "groupnorm_silu_quant", "layernorm_quant", "geglu_quant",
               "quantize_heads", "attn_i8", "attn_keyterm", "conv2d_i8_form", "bmm_qk_i8", "bmm_pv_i8", "temb_mlp")
CALL_FIELDS = ("ldx", "ldk", "ldo", "ldr", "ld_rowbias", "B", "H", "W", "Ho", "Wo", "Cout", "kh", "kw", "stride", "pad_t",
               "pad_l", "wbits", "epilogue", "splitk")
INT_CALL_FIELDS = CALL_FIELDS + ("w_tiled", "upsample2x", "res_period")


def _describe(a, fields=CALL_FIELDS):
    from qdiff import hip
    if torch.is_tensor(a):
        return [str(a.dtype).replace("torch.", ""), list(a.shape), list(a.stride())]
    if isinstance(a, hip.ConvCall):
        d = {k: _describe(getattr(a, k)) for k in fields}
        d.update({k: _describe(getattr(a, k)) for k in ("x", "out", "residual", "rowbias", "bias")})
        d["segs"] = [[s["c0"], s["clen"], s["kofs"], s.get("kstep0", 0)] for s in a.segs]
        if fields is INT_CALL_FIELDS:
            d["gn_part"] = _describe(a.gn_part)
        return d
    if isinstance(a, torch.dtype):
        return str(a).replace("torch.", "")
    if isinstance(a, (tuple, list)):
        return [_describe(v, fields) for v in a]
    if isinstance(a, float):
        return repr(a)
    if a is None or isinstance(a, (bool, int, str)):
        return a
    if hasattr(a, "Cout") and hasattr(a, "Cin"):               # a plan (the members of qd_temb_mlp_wq_h16)
        return [type(a).__name__, a.Cin, a.Cout]
    return type(a).__name__


def _install(mp, log):
    """The emulators of the host suites, stacked (mod producers, embedding Linears, GEGLU epilogue, fp64 attention), each entry
    point logged."""
    import wonly_mod_emulator
    import wonly_temb_emulator
    import wonly_wide_emulator
    from qdiff import hip
    from test_weight_only_attention_host import attn_h16_emulated
    wonly_mod_emulator.install(mp)
    wonly_temb_emulator.install(mp)
    mp.setattr(hip, "conv2d_wq_h16", wonly_wide_emulator.conv2d_wq_h16)
    mp.setattr(hip, "attn_h16", attn_h16_emulated)
    for name in SHAPED:
        def logged(*a, _fn=getattr(hip, name), _name=name):
            log.append([_name] + [_describe(v) for v in a])
            return _fn(*a)
        mp.setattr(hip, name, logged)


def _install_int(mp, log):
    """tests/cfg_pair_emulator.py (abi_emulator plus the two periods of a guidance pair), each computing entry point logged by
    name, the contractions with their ConvCall."""
    import cfg_pair_emulator
    from qdiff import hip
    cfg_pair_emulator.install(mp)
    for name in INT_ENTRIES:
        def logged(*a, _fn=getattr(hip, name), _name=name, **k):
            shaped = _name in ("conv2d_i8", "conv2d_i8_group")
            log.append([_name] + ([_describe(a[0], INT_CALL_FIELDS)] if shaped else []))
            return _fn(*a, **k)
        mp.setattr(hip, name, logged)


def _resume(name, dev):
    """The tiny / full golden model `name` with its calibrated quantisers, on `dev`; (model, fixture)."""
    import qdiff
    from golden_util import build_ckpt, build_engine_model, fixture_inputs, load_fixture, quant_params
    from qdiff.utils import resume_cali_model
    fx = load_fixture(f"model_{name}.pt")
    spec = fx["spec"]
    wq, aq = quant_params(spec)
    qnn = qdiff.QuantModel(build_engine_model(spec).to(dev), wq, aq, sm_abit=spec["sm_abit"]).to(dev).eval()
    cal = tuple(a.to(dev) for a in fixture_inputs(fx, "cal") if a is not None)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ckpt.pth")
        torch.save(build_ckpt(fx), path)
        resume_cali_model(qnn, path, cal, quant_act=True, cond=spec["ctx"] is not None)
    return qnn, fx


class _Counters:
    """The weights-only counters of one evaluation (the launch counters as differences)."""

    def __init__(self, mp):
        from qdiff import engine
        self.engine = engine
        mp.setattr(engine, "WONLY_FUSED", {"resblock": 0, "transformer": 0})
        mp.setattr(engine, "WONLY_GEGLU_EPI", [0])
        self.temb, self.attn = engine.WONLY_TEMB[0], engine.ATTN_H16_LAUNCHES

    def read(self):
        e = self.engine
        return dict(sorted(e.WONLY_FUSED.items()), geglu_epi=e.WONLY_GEGLU_EPI[0], temb=e.WONLY_TEMB[0] - self.temb,
                    attn_h16=e.ATTN_H16_LAUNCHES - self.attn)


def _entry(key, log, counters, y):
    y = y.detach().cpu().contiguous()
    blob = json.dumps(log, sort_keys=True).encode()
    r = dict(ncalls=len(log or ()), calls=hashlib.sha256(blob).hexdigest() if log is not None else "-", counters=counters,
             dtype=str(y.dtype), out=hashlib.sha256(y.numpy().tobytes()).hexdigest())
    print(key, r["ncalls"], r["counters"], r["out"][:12], flush=True)
    return r


def _set_knobs(engine, attn=None, fuse=0, wide=0, mod=0, ddim=0, temb=0):
    engine.set_weight_only_attention(attn)
    engine.set_weight_only_fusion(bool(fuse))
    engine.set_weight_only_fusion_wide(bool(wide))
    engine.set_weight_only_fusion_mod(bool(mod))
    engine.set_weight_only_fusion_ddim(bool(ddim))
    engine.set_weight_only_temb(bool(temb))


def _record_int(res):
    import pytest
    from qdiff import engine
    from golden_util import fixture_inputs
    mp, log = pytest.MonkeyPatch(), []
    try:
        _install_int(mp, log)
        mp.setattr(engine, "CFG_SHARE", True)
        for name in TINY + INT_FULL:
            qnn, fx = _resume(name, "cpu")
            qnn.set_quant_state(True, True)
            args = tuple(a for a in fixture_inputs(fx, "test") if a is not None)
            del log[:]
            with torch.no_grad():
                y = qnn(*args)
            res[f"{name} int"] = _entry(f"{name} int", log, {}, y)
            if name == "sd_tiny":
                # one sample duplicated the way a sampler does, a context of two distinct rows (uncond | cond), prepared up front
                x, t, c = fixture_inputs(fx, "test")
                x, t = torch.cat([x[:1]] * 2), torch.cat([t[:1]] * 2)
                c = torch.randn((2,) + tuple(c.shape[1:]), generator=torch.Generator().manual_seed(7))
                with torch.no_grad():
                    assert qnn.prepare_context(c)
                engine.mark_pair(x, t)
                del log[:]
                before = qnn.pair_evals
                with torch.no_grad():
                    y = qnn(x, t, c)
                res[f"{name} int pair"] = _entry(f"{name} int pair", log, {"pair_evals": qnn.pair_evals - before}, y)
    finally:
        mp.undo()


def record(path):
    import pytest
    from qdiff import engine
    from test_weight_only_fused_host import _model
    res = {}
    _record_int(res)
    mp, log = pytest.MonkeyPatch(), []
    try:
        _install(mp, log)
        engine.set_weight_only_kernel(torch.float16)
        for name in MODELS + DDIM_MODELS:
            qnn, args = _model(name)
            for attn in (None, torch.float16):
                at = "fp16" if attn else "off"
                if name in DDIM_MODELS:
                    cases = [(dict(fuse=f, ddim=d, temb=t), f"{name} fuse={f} ddim={d} temb={t} attn={at}") for f, d, t in DDIM_KNOBS]
                else:
                    cases = [(dict(fuse=f, wide=w, mod=m, temb=t), f"{name} fuse={f} wide={w} mod={m}{' temb=1' if t else ''} attn={at}")
                             for f, w, m, t in KNOBS]
                for knobs, key in cases:
                    _set_knobs(engine, attn, **knobs)
                    cnt = _Counters(mp)
                    del log[:]
                    with torch.no_grad():
                        y = qnn(*args)
                    res[key] = _entry(key, log, cnt.read(), y)
    finally:
        mp.undo()
        _set_knobs(engine)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def record_gpu(path):
    """The real library on cuda:0: no call list (the CPU record proves it), the counters and the output bytes."""
    import pytest
    from qdiff import engine
    from golden_util import fixture_inputs
    dev, mp, res = torch.device("cuda:0"), pytest.MonkeyPatch(), {}
    engine.set_weight_only_splitk(False)
    engine.set_weight_only_graph(False)
    try:
        for name in TINY:
            qnn, fx = _resume(name, dev)
            args = tuple(a.to(dev) for a in fixture_inputs(fx, "test") if a is not None)
            for state in ((True, True), (True, False)):
                qnn.set_quant_state(*state)
                for on in (0, 1):
                    engine.set_weight_only_kernel(torch.float16)
                    _set_knobs(engine, torch.float16 if on else None, on, on, on, on, on)
                    cnt = _Counters(mp)
                    for rep in (0, 1):                   # the first evaluation of a state plans and packs; the second is steady
                        with torch.no_grad():
                            y = qnn(*args)
                        torch.cuda.synchronize()
                        key = f"gpu {name} state={int(state[0])}{int(state[1])} knobs={'on' if on else 'kernel'} eval={rep}"
                        res[key] = _entry(key, None, cnt.read(), y)
    finally:
        mp.undo()
        engine.set_weight_only_kernel(None)
        _set_knobs(engine)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    print("model, knobs | call list: launches, SHA-256 (names, shape arguments, leading dimensions) | counters | "
          "output SHA-256; each column first record / second record, then 'equal' (any other word: the two records differ)")
    bad = 0
    for key in sorted(set(a) | set(b)):
        ra, rb = a.get(key), b.get(key)
        if ra is None or rb is None:
            print(f"{key:58s} missing in {'first' if ra is None else 'second'} record: DIFFERENT")
            bad += 1
            continue
        cols = []
        for what, fmt in (("calls", lambda r: f"{r['ncalls']} {r['calls'][:12]}"),
                          ("counters", lambda r: ",".join(f"{k}={v}" for k, v in r["counters"].items())),
                          ("out", lambda r: r["out"][:16])):
            same = fmt(ra) == fmt(rb) and ra[what] == rb[what]
            bad += not same
            cols.append(f"{fmt(ra)} / {fmt(rb)} {'equal' if same else 'DIFFERENT'}")
        print(f"{key:58s} " + " | ".join(cols))
    print(f"{len(set(a) | set(b))} cases, {bad} differing entries")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1:3] == ["record", "--gpu"]:
        record_gpu(sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
