#!/usr/bin/env python3
"""The first-stage decoder's mid-block attention (one head, 512 channels) on the library call and on qd_attn_h16_wide
(first_stage_hip.DECODER_ATTN = "library" / "hip"):

    attention alone   (B, T, C) = (1, 4096, 512)  (8, 4096, 512)  (4, 1024, 512)     SD latent, 8 SD latents, 4 LSUN-Churches
    whole decode      SD 512 x 512 (KL-f8, 4 x 64 x 64 latents, key-derived synthetic weights), batches --decode-batches

Both sides read the q | k | v column ranges of ONE [B*T][3C] tensor as HipDecoder._attn hands them over and produce proj_out's
operand rows [B*T][C] (the library side's reshape + contiguous included: it is part of what that route costs).  The sides are
alternated library / hip three times in ONE process after a warm-up of each; a window is `--iters` calls between two device
events.  Per side the best window and the spread of the three are printed, the achieved TFLOP/s (4 B T^2 C operations over the
best window) and the largest difference between the two results.  The report goes to --out as well.  GPU box:

    python tools/bench_decoder_attn.py [--iters 50] [--dtypes fp16,bf16] [--out profiles/decoder_attn.txt]

--rehearse runs the library side once on tiny tensors on the CPU (shapes and plumbing only: it prints no time)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
from qdiff import first_stage_hip as fh, hip, synthetic  # noqa: E402
from qdiff.arch import first_stage as fs  # noqa: E402

SHAPES = [(1, 4096, 512), (8, 4096, 512), (4, 1024, 512)]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def attention(qkv, B, T, C, side):
    """proj_out's operand rows [B*T][C] from the fused projection's rows [B*T][3C], as HipDecoder._attn computes them"""
    if side == "library":
        q, k, v = (qkv[:, i * C:(i + 1) * C].reshape(B, 1, T, C) for i in range(3))
        return F.scaled_dot_product_attention(q, k, v, scale=C ** -0.5).reshape(B * T, C).contiguous()
    st = (T * 3 * C, 3 * C, C, 1)
    o = torch.empty((B * T, C), dtype=qkv.dtype, device=qkv.device)
    hip.attn_h16_wide(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, T, T, 1, C, st, st, st, C ** -0.5, qkv.dtype, o)
    return o


def windows(fn, iters):
    """{side: [ms per call] of three windows}, sides alternated, one warm-up call of each side first"""
    for side in ("library", "hip"):
        fn(side)
    ms = {"library": [], "hip": []}
    for _ in range(3):
        for side in ("library", "hip"):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn(side)
            e1.record()
            torch.cuda.synchronize()
            ms[side].append(e0.elapsed_time(e1) / iters)
    return ms


def line(side, v, extra=""):
    return f"  {side:8s}: best {min(v):9.4f} ms  (three windows {', '.join(f'{x:.4f}' for x in v)}; spread {max(v) - min(v):.4f}){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--decode-iters", type=int, default=10)
    ap.add_argument("--decode-batches", default="1,8")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_attn.txt"))
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        for B, T, C in SHAPES:
            o = attention(torch.randn(B * 8, 3 * 16), B, 8, 16, "library")
            print(f"({B}, {T}, {C}): rehearsal at T = 8, C = 16, rows {tuple(o.shape)} (no timing on the CPU)")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_decoder_attn.py measures on the GPU: no device visible")
    dev = torch.device("cuda:0")
    rep = [f"# decoder mid-block attention, library (scaled_dot_product_attention) vs hip (qd_attn_h16_wide); {a.iters} calls per window "
           f"({a.decode_iters} decodes), sides alternated x3 in one process after one warm-up call each; device events; "
           f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}"]

    def say(s):
        print(s, flush=True)
        rep.append(s)

    alone = {}                                                   # (dtype, B) -> best ms of the 4096-token call, per side
    for name in a.dtypes.split(","):
        dt = DTYPES[name]
        for B, T, C in SHAPES:
            qkv = torch.randn(B * T, 3 * C, generator=torch.Generator().manual_seed(B * T + C)).to(dev, dt)
            lib, own = attention(qkv, B, T, C, "library"), attention(qkv, B, T, C, "hip")
            diff = (lib.float() - own.float()).abs().max().item() / lib.float().abs().max().item()
            ms = windows(lambda side: attention(qkv, B, T, C, side), a.iters)
            tf = lambda v: f"  {4.0 * B * T * T * C / min(v) / 1e9:7.1f} TFLOP/s"
            say(f"attention {name} (B, T, C) = ({B}, {T}, {C}): {(T + 31) // 32 * B} blocks of qd_attn_h16_wide for 256 CUs; "
                f"max |library - hip| = {diff:.2e} of the output range")
            say(line("library", ms["library"], tf(ms["library"])))
            say(line("hip", ms["hip"], tf(ms["hip"])))
            say(f"  library / hip = {min(ms['library']) / min(ms['hip']):.2f}x")
            if T == 4096:
                alone[(name, B)] = {side: min(v) for side, v in ms.items()}
            del qkv, lib, own
    m, _ = fs.sd_v1_first_stage()
    m.load_state_dict({k: synthetic.tensor_for(k, v.shape, seed=0) for k, v in m.state_dict().items()})
    m = m.eval().to(dev)
    for name in a.dtypes.split(","):
        for B in (int(b) for b in a.decode_batches.split(",")):
            with torch.no_grad():
                z = m.post_quant_conv(torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev)).float()
            dec = {side: fh.HipDecoder(m.decoder, DTYPES[name], attention=side) for side in ("library", "hip")}
            lib, own = dec["library"](z), dec["hip"](z)
            diff = (lib - own).abs().max().item() / lib.abs().max().item()
            ms = windows(lambda side: dec[side](z), a.decode_iters)
            say(f"decode {name} SD 512 x 512, batch {B} (ms per batch): max |library - hip| = {diff:.2e} of the image range")
            say(line("library", ms["library"]))
            say(line("hip", ms["hip"]))
            share = "; ".join(f"{side} {100 * alone[(name, B)][side] / min(ms[side]):.1f} %" for side in ms) if (name, B) in alone else "n/a"
            say(f"  library / hip = {min(ms['library']) / min(ms['hip']):.3f}x; the attention call's share of its decode (time alone over "
                f"decode time): {share}")
            del dec, lib, own
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(rep) + "\n")


if __name__ == "__main__":
    main()
