#!/usr/bin/env python3
"""Host-side record of the weights-only routes, for refactors that must not change them (CPU, on the emulators of tests/).

    python tools/wonly_route_bits.py record OUT.json          one tree: every model x knob combination below
    python tools/wonly_route_bits.py compare A.json B.json    two records -> one two-column line per case, 'equal' or not

Per case it keeps the call list of the emulated entry points of qdiff.hip (names; for the producers, qd_rows_to_h16 and the
contraction also every shape argument and leading dimension), the engine.WONLY_FUSED counters and a SHA-256 of the output
bytes.  Knob combinations: fusion / wide / modulated-resampling / fp16 attention, each on and off; wide and modulated without
the fusion knob are kept (the host tests hold them to "changes nothing"), wide together with modulated only under fusion."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "q-diffusion_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

MODELS = ("ldm_tiny", "ldm_updown_tiny", "sd_tiny", "churches_full")
# (fuse, wide, mod)
KNOBS = ((0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1))
SHAPED = ("rows_to_h16", "conv2d_wq_h16", "layernorm_h16", "geglu_h16", "groupnorm_h16", "groupnorm_mod_h16",
          "groupnorm_resample_h16", "attn_h16")
CALL_FIELDS = ("ldx", "ldk", "ldo", "ldr", "ld_rowbias", "B", "H", "W", "Ho", "Wo", "Cout", "kh", "kw", "stride", "pad_t",
               "pad_l", "wbits", "epilogue", "splitk")


def _describe(a):
    from qdiff import hip
    if torch.is_tensor(a):
        return [str(a.dtype).replace("torch.", ""), list(a.shape), list(a.stride())]
    if isinstance(a, hip.ConvCall):
        d = {k: getattr(a, k) for k in CALL_FIELDS}
        d.update({k: _describe(getattr(a, k)) for k in ("x", "out", "residual", "rowbias", "bias")})
        d["segs"] = [[s["c0"], s["clen"], s["kofs"], s.get("kstep0", 0)] for s in a.segs]
        return d
    if isinstance(a, torch.dtype):
        return str(a).replace("torch.", "")
    if isinstance(a, (tuple, list)):
        return [_describe(v) for v in a]
    if isinstance(a, float):
        return repr(a)
    return a


def _install(mp, log):
    """The emulators of the host suites, stacked (mod producers, GEGLU epilogue, fp64 attention), each entry point logged."""
    import wonly_mod_emulator
    import wonly_wide_emulator
    from qdiff import hip
    from test_weight_only_attention_host import attn_h16_emulated
    wonly_mod_emulator.install(mp)
    mp.setattr(hip, "conv2d_wq_h16", wonly_wide_emulator.conv2d_wq_h16)
    mp.setattr(hip, "attn_h16", attn_h16_emulated)
    for name in SHAPED:
        def logged(*a, _fn=getattr(hip, name), _name=name):
            log.append([_name] + [_describe(v) for v in a])
            return _fn(*a)
        mp.setattr(hip, name, logged)


def record(path):
    import pytest
    from qdiff import engine
    from test_weight_only_fused_host import _model
    mp, log, res = pytest.MonkeyPatch(), [], {}
    try:
        _install(mp, log)
        engine.set_weight_only_kernel(torch.float16)
        for name in MODELS:
            qnn, args = _model(name)
            for attn in (None, torch.float16):
                for fuse, wide, mod in KNOBS:
                    engine.set_weight_only_attention(attn)
                    engine.set_weight_only_fusion(bool(fuse))
                    engine.set_weight_only_fusion_wide(bool(wide))
                    engine.set_weight_only_fusion_mod(bool(mod))
                    mp.setattr(engine, "WONLY_FUSED", {"resblock": 0, "transformer": 0})
                    mp.setattr(engine, "WONLY_GEGLU_EPI", [0])
                    del log[:]
                    with torch.no_grad():
                        y = qnn(*args)
                    key = f"{name} fuse={fuse} wide={wide} mod={mod} attn={'fp16' if attn else 'off'}"
                    blob = json.dumps(log, sort_keys=True).encode()
                    res[key] = dict(ncalls=len(log), calls=hashlib.sha256(blob).hexdigest(),
                                    counters=dict(sorted(engine.WONLY_FUSED.items()), geglu_epi=engine.WONLY_GEGLU_EPI[0]),
                                    dtype=str(y.dtype), out=hashlib.sha256(y.contiguous().numpy().tobytes()).hexdigest())
                    print(key, res[key]["ncalls"], res[key]["counters"], res[key]["out"][:12], flush=True)
    finally:
        mp.undo()
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    print("model, knobs | call list: launches, SHA-256 (names, shape arguments, leading dimensions) | WONLY_FUSED counters | "
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
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
