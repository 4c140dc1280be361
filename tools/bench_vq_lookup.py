#!/usr/bin/env python3
"""The VQ head of the LDM-4 first stage (LSUN-Bedrooms: 8192 codes of 3 channels, 64 x 64 latents) with QDIFF_DECODER_VQ off
and on:

  (a) the head alone, latent -> conv_in's operand rows, at B x 4096 pixels for B in {1, 10, 16, 64}
        off: VectorQuantizer.forward (distance matrix, argmin, gather, permute) + post_quant_conv + .float() + the row
             conversion of HipDecoder._walk
        on : one qd_vq_lookup with the folded table (first_stage_hip.vq_rows)
  (b) a whole decode_first_stage(lsun_beds_first_stage(), engine="hip") at B = 1 and 10 (key-derived synthetic weights)

The knob is alternated off / on three times in ONE process after a warm-up of each side; a window is `--iters` calls between
two device events.  Per side the best window, the spread of the three and torch.cuda.max_memory_allocated of a call (above what
was allocated before it) are printed, then the launch form, the share of pixels on which both sides picked the same code, and
the box probe.  GPU box:

    python tools/bench_vq_lookup.py [--iters 20]

--rehearse runs the off side once on a tiny latent on the CPU (shapes and plumbing only: it prints no time)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
from qdiff import first_stage_hip as fh, hip, synthetic  # noqa: E402
from qdiff.arch import first_stage as fs  # noqa: E402


def model(dev, n_embed=8192):
    m, _ = fs.lsun_beds_first_stage()
    if n_embed != 8192:
        m = fs.VQModelDecoder(dict(double_z=False, z_channels=3, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2],
                                   num_res_blocks=1, attn_resolutions=[], dropout=0.0), embed_dim=3, n_embed=n_embed)
    m.load_state_dict({k: synthetic.tensor_for(k, v.shape, seed=0) for k, v in m.state_dict().items()})
    return m.eval().to(dev)


def head_off(m, z, hd):
    """what decode_first_stage and HipDecoder._walk do between the latent and conv_in with the knob off"""
    q = m.post_quant_conv(m.quantize(z)).float()
    B, zc, H, W = q.shape
    x0 = torch.zeros((B * H * W, hd.conv_in_width(z.device)), dtype=hd.dtype, device=z.device)
    x0[:, :zc] = q.permute(0, 2, 3, 1).reshape(B * H * W, zc)
    return x0


def windows(sides, iters):
    """{name: callable} -> {name: (three window means in ms, peak bytes of one call above the bytes held before it)}"""
    ms, peak = {k: [] for k in sides}, {}
    for name, fn in sides.items():                      # warm-up of each side, and its peak
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - held
    for _ in range(3):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    return {k: (ms[k], peak[k]) for k in sides}


def report(title, res):
    print(title)
    for name, (w, peak) in res.items():
        print(f"  {name:3s}: best {min(w):9.4f} ms  (three windows {', '.join(f'{v:.4f}' for v in w)}; spread {max(w) - min(w):.4f})  "
              f"peak memory of a call {peak / 2 ** 20:9.2f} MiB")
    off, on = res["off"][0], res["on"][0]
    verdict = "faster by more than the off side's spread" if min(off) - min(on) > max(off) - min(off) else "NOT faster by more than the off side's spread"
    print(f"  off / on = {min(off) / min(on):.2f}x: on is {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,10,16,64")
    ap.add_argument("--decode-batches", default="1,10")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        m = model(torch.device("cpu"), n_embed=64)
        with torch.no_grad():
            q = m.post_quant_conv(m.quantize(torch.randn(1, 3, 8, 8)))
        print(f"rehearsal: head on the CPU at 1 x 3 x 8 x 8, 64 codes -> {tuple(q.shape)} (no timing on the CPU)")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_vq_lookup.py measures on the GPU: no device visible")
    dev = torch.device("cuda:0")
    print(f"# VQ-f4 head, 8192 codes x 3 channels, {a.iters} calls per window after a warm-up call per side, knob alternated off/on x3 "
          f"in one process; device events; {torch.cuda.get_device_name(0)}")
    m = model(dev)
    hd = fh.hip_decoder(m.decoder)
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            z = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(B)).to(dev).contiguous(memory_format=torch.channels_last)
            fh.set_decoder_vq("library")
            rows_off = head_off(m, z, hd)
            fh.set_decoder_vq("hip")
            rows_on = fh.vq_rows(m, z, hd)
            same = (rows_off == rows_on).all(1).float().mean().item()

            def off():
                fh.set_decoder_vq("library")
                return head_off(m, z, hd)

            def on():
                fh.set_decoder_vq("hip")
                return fh.vq_rows(m, z, hd)

            slices, launches = hip.vq_lookup_form(B, 4096, 8192)
            report(f"(a) head alone, {B} x 4096 pixels: {slices} code slice(s), {launches} launch(es); rows equal on {100 * same:.3f} % of the pixels",
                   windows({"off": off, "on": on}, a.iters))
            del z, rows_off, rows_on
            torch.cuda.empty_cache()
        for B in [int(b) for b in a.decode_batches.split(",")]:
            z = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(100 + B)).to(dev)

            def dec(mode):
                fh.set_decoder_vq(mode)
                return fs.decode_first_stage(m, z, 1.0, engine="hip")

            a_off, a_on = dec("library"), dec("hip")
            dist = (a_off - a_on).abs().max().item() / a_off.abs().max().item()
            report(f"(b) decode_first_stage(lsun_beds, engine='hip'), batch {B}: on vs off max difference {dist:.3e} of range",
                   windows({"off": lambda: dec("library"), "on": lambda: dec("hip")}, max(1, a.iters // 4)))
            torch.cuda.empty_cache()
    fh.set_decoder_vq("library")
    ms, ticks = hip.box_probe(dev, 0, 512, 60000)
    print(f"# box probe (MFMA loop, 512 blocks x 60000 iterations): {ms:.3f} ms, {ticks:.0f} ticks")


if __name__ == "__main__":
    main()
