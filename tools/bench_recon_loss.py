#!/usr/bin/env python3
"""The reconstruction term of one calibration iteration — gather of the target rows, loss, backward to d loss / d pred — as the
ATen composition (engine.FUSED_RECON_LOSS off) and as the fused call (on), on unit outputs of SD size:

    o16x320x64x64       a 320-channel block output, batch 16, channels-last like its cache
    o8x1280x16x16       a 1280-channel block output
    t8x4096x320         a [B, T, C] transformer-unit output
    mixed16x320x64x64   pred channels-last, the cache NCHW (the tiled path)

each for 'mse' (p = 2) and 'fisher_diag', the cache holding 4 x the batch.  The two sides alternate three times in ONE process
after a warm-up of each; a window is `--iters` terms between two device events; per side the best window and the spread are
printed, with whether the gradients agree bit for bit and the error of both losses against fp64.  Then one weight-phase
iteration of the `res320` unit of tools/bench_adaround.py with the knob off and on.  GPU box:

    python tools/bench_recon_loss.py [--iters 50] [--shapes a,b] [--unit-iters 50]

--rehearse runs the composition once on tiny tensors on the CPU (shapes and plumbing only: it prints no time)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from qdiff import engine, recon  # noqa: E402

# (name, shape, pred channels-last, cache channels-last, tiny shape)
SHAPES = [("o16x320x64x64", (16, 320, 64, 64), True, True, (2, 8, 4, 4)),
          ("o8x1280x16x16", (8, 1280, 16, 16), True, True, (2, 8, 4, 4)),
          ("t8x4096x320", (8, 4096, 320), False, False, (2, 16, 8)),
          ("mixed16x320x64x64", (16, 320, 64, 64), True, False, (2, 8, 4, 4))]


def make(shape, pred_cl, cache_cl, dev):
    g = torch.Generator(device=dev).manual_seed(17)
    order = lambda t, cl: t.contiguous(memory_format=torch.channels_last) if cl else t
    rows = 4 * shape[0]
    cache = order(torch.randn((rows,) + shape[1:], generator=g, device=dev), cache_cl)
    gcache = order(torch.randn((rows,) + shape[1:], generator=g, device=dev), cache_cl)
    idx = torch.randperm(rows, generator=torch.Generator().manual_seed(5))[:shape[0]].to(dev)
    pred = order(cache[idx] + 0.05 * torch.randn(shape, generator=g, device=dev), pred_cl)
    return pred, cache, gcache, idx


def term(kind, pred, cache, gcache, idx, fused, dtype=torch.float32):
    """One term and its backward; off: the loop's gather and the composition.  Returns (loss, d loss / d pred)."""
    p = pred.detach().to(dtype).requires_grad_()
    engine.set_fused_recon_loss(fused)
    try:
        if fused:
            loss = recon._reconstruction_term(kind, p, (cache, idx), (gcache, idx), 2.0)
        else:
            loss = recon._reconstruction_term(kind, p, cache[idx].to(dtype), gcache[idx].to(dtype) if kind != "mse" else None, 2.0)
        loss.backward()
    finally:
        engine.set_fused_recon_loss(False)
    return loss.detach(), p.grad


def windows(run, iters):
    ms = {False: [], True: []}
    for rep in range(3):
        for fused in (False, True):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(fused, iters)
            e1.record()
            torch.cuda.synchronize()
            ms[fused].append(e0.elapsed_time(e1) / iters)
    return ms[False], ms[True]


def unit_iteration(iters, warmup):
    import bench_adaround as ba
    dev = torch.device("cuda:0")
    qnn, unit, args = ba.make_unit("res320", dev, tiny=False)
    tgt, params = ba.prepare(qnn, unit, args)
    init = [p.detach().clone() for p in params]

    def run(fused, n):
        with torch.no_grad():
            for p, p0 in zip(params, init):
                p.copy_(p0)
                p.grad = None
        engine.set_fused_recon_loss(fused)
        try:
            return ba.iterations(unit, args, tgt, params, n, fused=False)
        finally:
            engine.set_fused_recon_loss(False)
    calls = engine.RECON_LOSS_CALLS[0]
    losses = {fused: float(run(fused, warmup)) for fused in (False, True)}
    calls = engine.RECON_LOSS_CALLS[0] - calls
    off, on = windows(run, iters)
    print(f"res320 weight-phase iteration (batch {ba.BATCH}, FUSED_ADAROUND off), {iters} iterations per window; fused calls in the warm-up: {calls} of {warmup}")
    print(f"  off: best {min(off):8.3f} ms (spread {max(off) - min(off):.3f})   on: best {min(on):8.3f} ms (spread {max(on) - min(on):.3f})   "
          f"off / on = {min(off) / min(on):.3f}x, difference {min(off) - min(on):+.3f} ms   loss after warm-up off {losses[False]:.6f} on {losses[True]:.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--unit-iters", type=int, default=50)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    chosen = [s for s in SHAPES if s[0] in a.shapes.split(",")]
    if a.rehearse:
        for name, _, pcl, ccl, tiny in chosen:
            for kind in ("mse", "fisher_diag"):
                loss, g = term(kind, *make(tiny, pcl and len(tiny) == 4, ccl and len(tiny) == 4, torch.device("cpu")), False)
                print(f"{name} {kind}: rehearsal at {tiny}, loss {float(loss):.5f}, gradient {tuple(g.shape)} (no timing on the CPU)")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_recon_loss.py measures on the GPU: no device visible")
    dev = torch.device("cuda:0")
    print(f"# reconstruction term + backward to d loss / d pred, gather included; sides alternated off/on x3 in one process after one warm-up "
          f"term per side; {a.iters} terms per window; device events; {torch.cuda.get_device_name(0)}")
    for name, shape, pcl, ccl, _ in chosen:
        t = make(shape, pcl, ccl, dev)
        n = t[0].numel()
        print(f"{name}: {n / 1e6:.2f} M elements, pred {'channels-last' if pcl else 'dense'}, cache {'channels-last' if ccl else 'dense'}")
        for kind in ("mse", "fisher_diag"):
            (l_off, g_off), (l_on, g_on) = term(kind, *t, False), term(kind, *t, True)          # also the warm-up of each side
            l64 = float(term(kind, *t, False, torch.float64)[0])
            same = torch.equal(g_off.contiguous().view(torch.int32), g_on.contiguous().view(torch.int32))
            del g_off, g_on
            off, on = windows(lambda fused, k: [term(kind, *t, fused) for _ in range(k)], a.iters)
            need = 12 if kind == "mse" else 16
            print(f"  {kind:11s} off: best {min(off):8.3f} ms (spread {max(off) - min(off):.3f})   on: best {min(on):8.3f} ms (spread {max(on) - min(on):.3f})   "
                  f"off / on = {min(off) / min(on):.2f}x   on side: {n * need / min(on) / 1e6:.0f} GB/s of the {need} B/element it must move   "
                  f"bit-identical gradient: {same}   loss error / fp64: off {abs(float(l_off) - l64) / l64:.1e} on {abs(float(l_on) - l64) / l64:.1e}")
        del t
        torch.cuda.empty_cache()
    if a.unit_iters:
        unit_iteration(a.unit_iters, 3)


if __name__ == "__main__":
    main()
