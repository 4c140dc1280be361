"""Weights-only UNet evaluations (state (weight_quant, act_quant) = (True, False)): the time of one evaluation with the
weights-only kernel off (the reference's path: fake-quantised fp32 weights through the library convolutions, in fp32 and
under fp16 autocast) and on (qd_conv2d_wq_h16 on the packed codes with fp16 / bf16 activations), plus the contraction
class alone under HIP events and its share of the ~2.5 PF dense fp16 MFMA rate.  Same random-init models and inputs as
bench.py (SD-v1.4 at batch 16 by default).  One JSON line per model.

    python tools/bench_weight_only.py [--models sd,ldm,cifar] [--batch 16] [--evals 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
sys.path.insert(0, ROOT)

F16_MFMA_PEAK_TFLOPS = 2500.0      # dense fp16 / bf16 MFMA (MI355X_MICROARCH.md chip-level parameters)


def _timed(fn, k, warm=2):
    with torch.no_grad():
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / k


def _contraction_class(fn):
    """(ms, TFLOP) of the qd_conv2d_wq_h16 launches of one evaluation, each bracketed by HIP events."""
    from qdiff import hip
    orig, marks = hip.conv2d_wq_h16, []

    def timed(c, act_dtype):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        orig(c, act_dtype)
        b.record()
        K = c.kh * c.kw * sum(s["clen"] for s in c.segs)
        marks.append((a, b, 2.0 * c.B * c.Ho * c.Wo * c.Cout * K))
    hip.conv2d_wq_h16 = timed
    try:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
    finally:
        hip.conv2d_wq_h16 = orig
    return sum(a.elapsed_time(b) for a, b, _ in marks), sum(f for _, _, f in marks) / 1e12, len(marks)


def run(kind, batch, k, dev):
    import bench
    from qdiff import engine, synthetic
    qnn, _ = bench.build_quantised_unet(kind, dev)
    x, t, c = synthetic.synthetic_inputs(kind, batch, seed=0)
    args = [a.to(dev) for a in (x, t, c) if a is not None]
    qnn.set_quant_state(True, False)
    one = lambda: qnn(*args)
    res = {"model": kind, "batch": batch, "evals_timed": k}
    prev = engine.WEIGHT_ONLY_KERNEL
    try:
        engine.set_weight_only_kernel(None)
        res["off_fp32_ms"] = round(_timed(one, k), 3)
        with torch.autocast("cuda", dtype=torch.float16):
            res["off_autocast_fp16_ms"] = round(_timed(one, k), 3)
        for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            engine.set_weight_only_kernel(dt)
            res[f"on_{name}_ms"] = round(_timed(one, k), 3)
            ms, tflop, n = _contraction_class(one)
            res[f"on_{name}_contraction_ms"] = round(ms, 3)
            res[f"on_{name}_contraction_launches"] = n
            res[f"on_{name}_contraction_frac_of_peak"] = round(tflop / (ms / 1000.0) / F16_MFMA_PEAK_TFLOPS, 4) if ms > 0 else None
        res["speedup_fp16_vs_off_fp32"] = round(res["off_fp32_ms"] / res["on_fp16_ms"], 2)
    finally:
        engine.set_weight_only_kernel(prev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="sd,ldm,cifar")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--evals", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from qdiff import hip
    hip.load()
    dev = torch.device("cuda:0")
    for kind in a.models.split(","):
        print(json.dumps(run(kind, a.batch, a.evals, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
