"""Weights-only UNet evaluations (state (weight_quant, act_quant) = (True, False)): the time of one evaluation with the
weights-only kernel off (the reference's path: fake-quantised fp32 weights through the library convolutions, in fp32 and
under fp16 autocast) and on (qd_conv2d_wq_h16 on the packed codes with fp16 / bf16 activations), plus the contraction
class alone under HIP events and its share of the ~2.5 PF dense fp16 MFMA rate.  Same random-init models and inputs as
bench.py (SD-v1.4 at batch 16 by default).  One JSON line per model.

    python tools/bench_weight_only.py [--models sd,ldm,cifar] [--batch 16] [--evals 3]

--attn adds the attention-knob column (engine.WEIGHT_ONLY_ATTN, qd_attn_h16) with the layer kernel at fp16: evaluation time
with the fused attention off and on (alternated A/B in one process), the attention class (HIP events around every
engine.attention_h16 call; with the knob off, the library's fp32 attention core — einsum, * scale, softmax, einsum — timed in
isolation at the shapes the evaluation hits), torch.cuda.max_memory_allocated of one evaluation, and --attn-shapes a per-shape
table at SD's shapes (kernel us, TFLOP/s, share of the fp16 peak at 4*BH*T*S*d FLOP, F.scaled_dot_product_attention in fp16
and the library core in fp32 as yardsticks).

    python tools/bench_weight_only.py --attn [--models sd,ldm,churches] [--attn-shapes]

--fuse adds the block-fusion column (engine.WEIGHT_ONLY_FUSE) with the layer kernel at fp16 (and, with --attn, the attention
kernel at fp16): evaluation time with the fusion off and on, alternated A/B --rounds times in one process, best and spread of
each side, the blocks that took the fused route, peak memory, and a box probe (hip.box_probe) so that two runs can be told
apart.  --fuse-shapes prints the three producers alone at SD's shapes: microseconds and achieved GB/s (bytes read + written)
next to a plain device copy of the same bytes and the ~6.3 TB/s streaming ceiling.

    python tools/bench_weight_only.py --attn --fuse [--models sd,ldm] [--rounds 3] [--fuse-shapes]

--splitk: every other weights-only knob on (layer and attention kernels at fp16, fusion, wide fusion) and
engine.WEIGHT_ONLY_SPLITK off / on alternated --rounds times in one process: best, all values and spread of each side, the
launches that split, the distance of the outputs.  --splitk-shapes: the under-filled contraction shapes of SD-v1.4 and LDM-4
at batch 16 alone (HIP events, median and min..max of 3 repeats of 20 launches): the unsplit launch against forced slice counts
(hip.wq_h16_config, finalise included) and against the library's policy.

    python tools/bench_weight_only.py --splitk [--models sd,ldm,cifar] [--rounds 3] [--splitk-shapes]

--mod: layer kernel at fp16 and fusion on (with --attn the attention kernel, with --wide the wide fusion too), and
engine.WEIGHT_ONLY_FUSE_MOD off / on alternated --rounds times in one process: best, all values and spread of each side, the
blocks on the route, the distance of the outputs, peak memory, a box probe.  --mod-shapes: the three new launch forms alone at
LSUN-Churches' shapes at batch 16 (scale-shift norm; norm + 2x2 average; norm + nearest 2x) next to today's passes over the same
tensors and a device copy of the same bytes.

    python tools/bench_weight_only.py --attn --fuse --wide --mod --models churches [--rounds 3] [--mod-shapes]

--graph: every block-level weights-only knob on; the eager walk and the HIP-graph replay
(engine.WEIGHT_ONLY_GRAPH) alternated --rounds times in one process, best, all values and spread of each side; with --temb the
replay with the one-launch embedding Linears (engine.WEIGHT_ONLY_TEMB) as a third side; --temb alone alternates that knob on the
eager walk.  Also the launch count of one evaluation with and without TEMB and the outputs' agreement.

    python tools/bench_weight_only.py --attn --graph --temb --models cifar --batch 64 [--rounds 3]
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


def _events_ms(fn, k=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(k):
            fn()
        b.record()
        torch.cuda.synchronize()
    return a.elapsed_time(b) / k


def _library_core(BH, T, S, d, dev):
    """The reference's fp32 attention core at one shape (cross_attn_forward's einsum, * scale, softmax, einsum)."""
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = (torch.randn(BH, n, d, device=dev, generator=g) for n in (T, S, S))
    scale = d ** -0.5

    def core():
        sim = torch.einsum("b i d, b j d -> b i j", q, k) * scale
        return torch.einsum("b i j, b j d -> b i d", sim.softmax(dim=-1), v)
    return core


def _attention_class(one):
    """(ms, launches, shapes) of the engine.attention_h16 calls of one evaluation, each bracketed by HIP events."""
    from qdiff import engine
    orig, marks = engine.attention_h16, []

    def timed(q, k, v, B, T, S, H, d, *rest, **kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = orig(q, k, v, B, T, S, H, d, *rest, **kw)
        b.record()
        marks.append((a, b, (B * H, T, S, d)))
        return out
    engine.attention_h16 = timed
    try:
        with torch.no_grad():
            one()
        torch.cuda.synchronize()
    finally:
        engine.attention_h16 = orig
    return sum(a.elapsed_time(b) for a, b, _ in marks), len(marks), [s for _, _, s in marks]


def run_attn(kind, batch, k, dev):
    import bench
    from qdiff import engine, synthetic
    qnn, _ = bench.build_quantised_unet(kind, dev)
    x, t, c = synthetic.synthetic_inputs(kind, batch, seed=0)
    args = [a.to(dev) for a in (x, t, c) if a is not None]
    qnn.set_quant_state(True, False)
    one = lambda: qnn(*args)
    res = {"model": kind, "batch": batch, "layer_knob": "fp16", "evals_timed": k}
    prev_k, prev_a = engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN
    try:
        engine.set_weight_only_kernel(torch.float16)
        off, on = [], []
        for _ in range(3):                                       # alternated A/B
            engine.set_weight_only_attention(None)
            off.append(_timed(one, k))
            engine.set_weight_only_attention(torch.float16)
            on.append(_timed(one, k))
        res["attn_off_ms"], res["attn_on_ms"] = round(min(off), 3), round(min(on), 3)
        res["attn_off_ms_all"], res["attn_on_ms_all"] = [round(v, 3) for v in off], [round(v, 3) for v in on]
        ms, n, shapes = _attention_class(one)
        res["attn_on_class_ms"], res["attn_launches"] = round(ms, 3), n
        lib = sum(_events_ms(_library_core(BH, T, S, d, dev), 3) for BH, T, S, d in shapes)
        res["attn_off_class_ms"] = round(lib, 3)
        res["attn_off_class_share"] = round(lib / res["attn_off_ms"], 3)
        for name, dt in (("off", None), ("on", torch.float16)):
            engine.set_weight_only_attention(dt)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            with torch.no_grad():
                one()
            torch.cuda.synchronize()
            res[f"attn_{name}_max_mem_mib"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)
        res["shapes"] = sorted(set(shapes))
    finally:
        engine.set_weight_only_kernel(prev_k)
        engine.set_weight_only_attention(prev_a)
    return res


def run_fuse(kind, batch, k, dev, attn, rounds):
    import bench
    from qdiff import engine, hip, synthetic
    qnn, _ = bench.build_quantised_unet(kind, dev)
    x, t, c = synthetic.synthetic_inputs(kind, batch, seed=0)
    args = [a.to(dev) for a in (x, t, c) if a is not None]
    qnn.set_quant_state(True, False)
    one = lambda: qnn(*args)
    res = {"model": kind, "batch": batch, "layer_knob": "fp16", "attn_knob": "fp16" if attn else "off", "evals_timed": k, "rounds": rounds}
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE)
    try:
        engine.set_weight_only_kernel(torch.float16)
        engine.set_weight_only_attention(torch.float16 if attn else None)
        ms, ticks = hip.box_probe(dev, 0, 512, 60000)
        res["box_probe_mfma_ms"] = round(ms, 3)
        off, on = [], []
        for _ in range(rounds):                                  # alternated A/B
            engine.set_weight_only_fusion(False)
            off.append(_timed(one, k))
            engine.set_weight_only_fusion(True)
            on.append(_timed(one, k))
        res["fuse_off_ms"], res["fuse_on_ms"] = round(min(off), 3), round(min(on), 3)
        res["fuse_off_ms_all"], res["fuse_on_ms_all"] = [round(v, 3) for v in off], [round(v, 3) for v in on]
        res["fuse_off_spread_ms"], res["fuse_on_spread_ms"] = round(max(off) - min(off), 3), round(max(on) - min(on), 3)
        res["faster_by_more_than_spread"] = bool(min(off) - max(on) > 0 and min(off) - min(on) > max(max(off) - min(off), max(on) - min(on)))
        for k2 in engine.WONLY_FUSED:
            engine.WONLY_FUSED[k2] = 0
        with torch.no_grad():
            y_on = one()
        res["blocks_fused"] = dict(engine.WONLY_FUSED)
        engine.set_weight_only_fusion(False)
        with torch.no_grad():
            y_off = one()
        res["fuse_on_vs_off_of_range"] = float((y_on - y_off).abs().max() / y_off.abs().max())
        for name, flag in (("off", False), ("on", True)):
            engine.set_weight_only_fusion(flag)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            with torch.no_grad():
                one()
            torch.cuda.synchronize()
            res[f"fuse_{name}_max_mem_mib"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)
    finally:
        engine.set_weight_only_kernel(prev[0])
        engine.set_weight_only_attention(prev[1])
        engine.set_weight_only_fusion(prev[2])
    return res


def run_wide(kind, batch, k, dev, attn, rounds):
    """Layer knob fp16, block fusion on, engine.WEIGHT_ONLY_FUSE_WIDE off / on alternated `rounds` times in one process."""
    import bench
    from qdiff import engine, hip, synthetic
    qnn, _ = bench.build_quantised_unet(kind, dev)
    x, t, c = synthetic.synthetic_inputs(kind, batch, seed=0)
    args = [a.to(dev) for a in (x, t, c) if a is not None]
    qnn.set_quant_state(True, False)
    one = lambda: qnn(*args)
    res = {"model": kind, "batch": batch, "layer_knob": "fp16", "attn_knob": "fp16" if attn else "off", "fuse": True, "evals_timed": k, "rounds": rounds}
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_FUSE_WIDE)
    try:
        engine.set_weight_only_kernel(torch.float16)
        engine.set_weight_only_attention(torch.float16 if attn else None)
        engine.set_weight_only_fusion(True)
        ms, ticks = hip.box_probe(dev, 0, 512, 60000)
        res["box_probe_mfma_ms"] = round(ms, 3)
        off, on = [], []
        for _ in range(rounds):                                  # alternated A/B
            engine.set_weight_only_fusion_wide(False)
            off.append(_timed(one, k))
            engine.set_weight_only_fusion_wide(True)
            on.append(_timed(one, k))
        res["wide_off_ms"], res["wide_on_ms"] = round(min(off), 3), round(min(on), 3)
        res["wide_off_ms_all"], res["wide_on_ms_all"] = [round(v, 3) for v in off], [round(v, 3) for v in on]
        res["wide_off_spread_ms"], res["wide_on_spread_ms"] = round(max(off) - min(off), 3), round(max(on) - min(on), 3)
        res["faster_by_more_than_spread"] = bool(min(off) - max(on) > 0 and min(off) - min(on) > max(max(off) - min(off), max(on) - min(on)))
        outs = {}
        for name, flag in (("off", False), ("on", True)):
            engine.set_weight_only_fusion_wide(flag)
            engine.WONLY_FUSED.pop("spatial", None)
            engine.WONLY_FUSED.pop("attnblock", None)
            for k2 in engine.WONLY_FUSED:
                engine.WONLY_FUSED[k2] = 0
            engine.WONLY_GEGLU_EPI[0] = 0
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            with torch.no_grad():
                outs[name] = one()
            torch.cuda.synchronize()
            res[f"wide_{name}_max_mem_mib"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)
            res[f"wide_{name}_blocks"] = dict(engine.WONLY_FUSED, geglu_epilogues=engine.WONLY_GEGLU_EPI[0])
        res["wide_on_vs_off_of_range"] = float((outs["on"] - outs["off"]).abs().max() / outs["off"].abs().max())
    finally:
        engine.set_weight_only_kernel(prev[0])
        engine.set_weight_only_attention(prev[1])
        engine.set_weight_only_fusion(prev[2])
        engine.set_weight_only_fusion_wide(prev[3])
        engine.WONLY_FUSED.pop("spatial", None)
        engine.WONLY_FUSED.pop("attnblock", None)
    return res


def run_splitk(kind, batch, k, dev, rounds):
    """Layer and attention kernels at fp16, fusion and wide fusion on; engine.WEIGHT_ONLY_SPLITK off / on alternated."""
    import bench
    from qdiff import engine, hip, synthetic
    qnn, _ = bench.build_quantised_unet(kind, dev)
    x, t, c = synthetic.synthetic_inputs(kind, batch, seed=0)
    args = [a.to(dev) for a in (x, t, c) if a is not None]
    qnn.set_quant_state(True, False)
    one = lambda: qnn(*args)
    res = {"model": kind, "batch": batch, "layer_knob": "fp16", "attn_knob": "fp16", "fuse": True, "wide": True, "evals_timed": k, "rounds": rounds}
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_FUSE_WIDE, engine.WEIGHT_ONLY_SPLITK)
    try:
        engine.set_weight_only_kernel(torch.float16)
        engine.set_weight_only_attention(torch.float16)
        engine.set_weight_only_fusion(True)
        engine.set_weight_only_fusion_wide(True)
        ms, ticks = hip.box_probe(dev, 0, 512, 60000)
        res["box_probe_mfma_ms"] = round(ms, 3)
        off, on = [], []
        for _ in range(rounds):                                  # alternated A/B
            engine.set_weight_only_splitk(False)
            off.append(_timed(one, k))
            engine.set_weight_only_splitk(True)
            on.append(_timed(one, k))
        res["splitk_off_ms"], res["splitk_on_ms"] = round(min(off), 3), round(min(on), 3)
        res["splitk_off_ms_all"], res["splitk_on_ms_all"] = [round(v, 3) for v in off], [round(v, 3) for v in on]
        res["splitk_off_spread_ms"], res["splitk_on_spread_ms"] = round(max(off) - min(off), 3), round(max(on) - min(on), 3)
        res["faster_by_more_than_spread"] = bool(min(off) - max(on) > 0 and min(off) - min(on) > max(max(off) - min(off), max(on) - min(on)))
        outs = {}
        for name, flag in (("off", False), ("on", True)):
            engine.set_weight_only_splitk(flag)
            engine.WONLY_SPLITK[0] = 0
            ms, tflop, n = _contraction_class(one)
            res[f"splitk_{name}_contraction_ms"], res[f"splitk_{name}_contraction_launches"] = round(ms, 3), n
            res[f"splitk_{name}_split_launches"] = engine.WONLY_SPLITK[0]
            with torch.no_grad():
                outs[name] = one()
        res["splitk_on_vs_off_of_range"] = float((outs["on"] - outs["off"]).abs().max() / outs["off"].abs().max())
    finally:
        engine.set_weight_only_kernel(prev[0])
        engine.set_weight_only_attention(prev[1])
        engine.set_weight_only_fusion(prev[2])
        engine.set_weight_only_fusion_wide(prev[3])
        engine.set_weight_only_splitk(prev[4])
    return res


def run_mod(kind, batch, k, dev, attn, wide, rounds):
    """Layer knob fp16, block fusion on; engine.WEIGHT_ONLY_FUSE_MOD off / on alternated `rounds` times in one process."""
    import bench
    from qdiff import engine, hip, synthetic
    qnn, _ = bench.build_quantised_unet(kind, dev)
    x, t, c = synthetic.synthetic_inputs(kind, batch, seed=0)
    args = [a.to(dev) for a in (x, t, c) if a is not None]
    qnn.set_quant_state(True, False)
    one = lambda: qnn(*args)
    res = {"model": kind, "batch": batch, "layer_knob": "fp16", "attn_knob": "fp16" if attn else "off", "fuse": True, "wide": bool(wide),
           "evals_timed": k, "rounds": rounds}
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_FUSE_WIDE, engine.WEIGHT_ONLY_FUSE_MOD)
    try:
        engine.set_weight_only_kernel(torch.float16)
        engine.set_weight_only_attention(torch.float16 if attn else None)
        engine.set_weight_only_fusion(True)
        engine.set_weight_only_fusion_wide(bool(wide))
        res["box_probe_mfma_ms"] = round(hip.box_probe(dev, 0, 512, 60000)[0], 3)
        off, on = [], []
        for _ in range(rounds):                                  # alternated A/B
            engine.set_weight_only_fusion_mod(False)
            off.append(_timed(one, k))
            engine.set_weight_only_fusion_mod(True)
            on.append(_timed(one, k))
        res["box_probe_mfma_ms_after"] = round(hip.box_probe(dev, 0, 512, 60000)[0], 3)
        res["mod_off_ms"], res["mod_on_ms"] = round(min(off), 3), round(min(on), 3)
        res["mod_off_ms_all"], res["mod_on_ms_all"] = [round(v, 3) for v in off], [round(v, 3) for v in on]
        res["mod_off_spread_ms"], res["mod_on_spread_ms"] = round(max(off) - min(off), 3), round(max(on) - min(on), 3)
        res["faster_by_more_than_spread"] = bool(min(off) - max(on) > 0 and min(off) - min(on) > max(max(off) - min(off), max(on) - min(on)))
        outs = {}
        for name, flag in (("off", False), ("on", True)):
            engine.set_weight_only_fusion_mod(flag)
            for key in ("resblock_mod", "spatial", "attnblock"):
                engine.WONLY_FUSED.pop(key, None)
            for k2 in engine.WONLY_FUSED:
                engine.WONLY_FUSED[k2] = 0
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            with torch.no_grad():
                outs[name] = one()
            torch.cuda.synchronize()
            res[f"mod_{name}_max_mem_mib"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)
            res[f"mod_{name}_blocks"] = dict(engine.WONLY_FUSED)
        res["mod_on_vs_off_of_range"] = float((outs["on"] - outs["off"]).abs().max() / outs["off"].abs().max())
    finally:
        engine.set_weight_only_kernel(prev[0])
        engine.set_weight_only_attention(prev[1])
        engine.set_weight_only_fusion(prev[2])
        engine.set_weight_only_fusion_wide(prev[3])
        engine.set_weight_only_fusion_mod(prev[4])
        for key in ("resblock_mod", "spatial", "attnblock"):
            engine.WONLY_FUSED.pop(key, None)
    return res


def run_ddim(kind, batch, k, dev, attn, rounds):
    """Every other weights-only knob on (layer knob fp16, block fusion, wide, mod, split-K; the attention knob with --attn);
    engine.WEIGHT_ONLY_FUSE_DDIM off / on alternated `rounds` times in one process."""
    import bench
    from qdiff import engine, hip, synthetic
    qnn, _ = bench.build_quantised_unet(kind, dev)
    x, t, c = synthetic.synthetic_inputs(kind, batch, seed=0)
    args = [a.to(dev) for a in (x, t, c) if a is not None]
    qnn.set_quant_state(True, False)
    one = lambda: qnn(*args)
    res = {"model": kind, "batch": batch, "layer_knob": "fp16", "attn_knob": "fp16" if attn else "off", "fuse": True, "wide": True,
           "mod": True, "splitk": True, "evals_timed": k, "rounds": rounds}
    prev = (engine.WEIGHT_ONLY_KERNEL, engine.WEIGHT_ONLY_ATTN, engine.WEIGHT_ONLY_FUSE, engine.WEIGHT_ONLY_FUSE_WIDE, engine.WEIGHT_ONLY_FUSE_MOD,
            engine.WEIGHT_ONLY_SPLITK, engine.WEIGHT_ONLY_FUSE_DDIM)
    new_keys = ("resnetblock", "attnblock_ddim", "head_ddim")
    try:
        engine.set_weight_only_kernel(torch.float16)
        engine.set_weight_only_attention(torch.float16 if attn else None)
        engine.set_weight_only_fusion(True)
        engine.set_weight_only_fusion_wide(True)
        engine.set_weight_only_fusion_mod(True)
        engine.set_weight_only_splitk(True)
        res["box_probe_mfma_ms"] = round(hip.box_probe(dev, 0, 512, 60000)[0], 3)
        off, on = [], []
        for _ in range(rounds):                                  # alternated A/B
            engine.set_weight_only_fusion_ddim(False)
            off.append(_timed(one, k))
            engine.set_weight_only_fusion_ddim(True)
            on.append(_timed(one, k))
        res["box_probe_mfma_ms_after"] = round(hip.box_probe(dev, 0, 512, 60000)[0], 3)
        res["ddim_off_ms"], res["ddim_on_ms"] = round(min(off), 3), round(min(on), 3)
        res["ddim_off_ms_all"], res["ddim_on_ms_all"] = [round(v, 3) for v in off], [round(v, 3) for v in on]
        res["ddim_off_spread_ms"], res["ddim_on_spread_ms"] = round(max(off) - min(off), 3), round(max(on) - min(on), 3)
        res["faster_by_more_than_spread"] = bool(min(off) - max(on) > 0 and min(off) - min(on) > max(max(off) - min(off), max(on) - min(on)))
        outs = {}
        for name, flag in (("off", False), ("on", True)):
            engine.set_weight_only_fusion_ddim(flag)
            for key in new_keys:
                engine.WONLY_FUSED.pop(key, None)
            for k2 in engine.WONLY_FUSED:
                engine.WONLY_FUSED[k2] = 0
            n0 = engine.ATTN_H16_LAUNCHES
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            with torch.no_grad():
                outs[name] = one()
            torch.cuda.synchronize()
            res[f"ddim_{name}_max_mem_mib"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)
            res[f"ddim_{name}_blocks"] = dict(engine.WONLY_FUSED)
            res[f"ddim_{name}_attn_launches"] = engine.ATTN_H16_LAUNCHES - n0
        res["ddim_on_vs_off_of_range"] = float((outs["on"] - outs["off"]).abs().max() / outs["off"].abs().max())
    finally:
        engine.set_weight_only_kernel(prev[0])
        engine.set_weight_only_attention(prev[1])
        engine.set_weight_only_fusion(prev[2])
        engine.set_weight_only_fusion_wide(prev[3])
        engine.set_weight_only_fusion_mod(prev[4])
        engine.set_weight_only_splitk(prev[5])
        engine.set_weight_only_fusion_ddim(prev[6])
        for key in new_keys:
            engine.WONLY_FUSED.pop(key, None)
    return res


def run_graph(kind, batch, k, dev, attn, temb, rounds):
    """Every block-level weights-only knob on (layer knob fp16, block fusion, wide, mod, DDIM, split-K; the attention knob with
    --attn).  --graph: engine.WEIGHT_ONLY_GRAPH off / on (eager walk / HIP-graph replay) alternated `rounds` times in one process,
    engine.WEIGHT_ONLY_TEMB as --temb says.  --graph --temb: under replay, engine.WEIGHT_ONLY_TEMB off / on alternated as well
    (the knob selects the graph: both stay captured).  --temb alone: the eager walk, TEMB off / on alternated.
    `launches` counts the calls of the library's launch wrappers during one eager walk (the replayed graph holds the same)."""
    import bench
    from qdiff import engine, hip, synthetic
    qnn, _ = bench.build_quantised_unet(kind, dev)
    x, t, c = synthetic.synthetic_inputs(kind, batch, seed=0)
    args = [a.to(dev) for a in (x, t, c) if a is not None]
    qnn.set_quant_state(True, False)
    one = lambda: qnn(*args)
    graph = "graph" in temb[1]
    res = {"model": kind, "batch": batch, "layer_knob": "fp16", "attn_knob": "fp16" if attn else "off", "fuse": True, "wide": True,
           "mod": True, "ddim": True, "splitk": True, "evals_timed": k, "rounds": rounds}
    names = ("WEIGHT_ONLY_KERNEL", "WEIGHT_ONLY_ATTN", "WEIGHT_ONLY_FUSE", "WEIGHT_ONLY_FUSE_WIDE", "WEIGHT_ONLY_FUSE_MOD",
             "WEIGHT_ONLY_FUSE_DDIM", "WEIGHT_ONLY_SPLITK", "WEIGHT_ONLY_TEMB", "WEIGHT_ONLY_GRAPH")
    prev = {n: getattr(engine, n) for n in names}

    def launches():
        wrappers = [n for n in ("conv2d_wq_h16", "rows_to_h16", "groupnorm_h16", "groupnorm_mod_h16", "groupnorm_resample_h16",
                                "layernorm_h16", "geglu_h16", "attn_h16", "temb_mlp_wq_h16") if hasattr(hip, n)]
        orig, n = {w: getattr(hip, w) for w in wrappers}, [0]
        for w in wrappers:
            setattr(hip, w, (lambda f: lambda *a, **kw: (n.__setitem__(0, n[0] + 1), f(*a, **kw))[1])(orig[w]))
        try:
            with torch.no_grad():
                one()
            torch.cuda.synchronize()
        finally:
            for w in wrappers:
                setattr(hip, w, orig[w])
        return n[0]

    try:
        engine.set_weight_only_kernel(torch.float16)
        engine.set_weight_only_attention(torch.float16 if attn else None)
        for f in (engine.set_weight_only_fusion, engine.set_weight_only_fusion_wide, engine.set_weight_only_fusion_mod,
                  engine.set_weight_only_fusion_ddim, engine.set_weight_only_splitk):
            f(True)
        sides = {}                                               # name -> (graph, temb)
        if graph:
            sides["eager"], sides["replay"] = (False, temb[0]), (True, temb[0])
            if temb[0]:
                sides["eager"], sides["replay"] = (False, False), (True, False)
                sides["replay_temb"] = (True, True)
        else:
            sides["temb_off"], sides["temb_on"] = (False, False), (False, True)
        qnn.enable_hip_graphs(True)                              # capture on first sight; only the knob decides whether anything is captured
        times = {name: [] for name in sides}
        res["box_probe_mfma_ms"] = round(hip.box_probe(dev, 0, 512, 60000)[0], 3)
        for _ in range(rounds):                                  # alternated
            for name, (g, te) in sides.items():
                engine.set_weight_only_graph(g)
                engine.set_weight_only_temb(te)
                times[name].append(_timed(one, k))
        res["box_probe_mfma_ms_after"] = round(hip.box_probe(dev, 0, 512, 60000)[0], 3)
        res["graphs_kept"] = len(qnn._graphs)
        for name, v in times.items():
            res[f"{name}_ms"], res[f"{name}_ms_all"] = round(min(v), 3), [round(u, 3) for u in v]
            res[f"{name}_spread_ms"] = round(max(v) - min(v), 3)
        outs = {}
        engine.set_weight_only_graph(False)
        for name, (g, te) in sides.items():
            engine.set_weight_only_graph(g)
            engine.set_weight_only_temb(te)
            with torch.no_grad():
                outs[name] = one().clone()
        torch.cuda.synchronize()
        engine.set_weight_only_graph(False)
        for te in sorted({te for _, te in sides.values()}):
            engine.set_weight_only_temb(te)
            res[f"launches_temb_{'on' if te else 'off'}"] = launches()
        first = next(iter(sides))
        for name in list(sides)[1:]:
            res[f"{name}_vs_{first}_of_range"] = float((outs[name] - outs[first]).abs().max() / outs[first].abs().max())
    finally:
        qnn.enable_hip_graphs(False)
        for n, v in prev.items():
            setattr(engine, n, v)
    return res


# the one-head attention of the CIFAR-10 DDIM UNet at batch 64: (B, T, d) of the five 16x16 blocks and of mid.attn_1
DDIM_ATTN_SHAPES = [(64, 256, 256), (64, 16, 256)]


def ddim_shape_table(dev, shapes=DDIM_ATTN_SHAPES):
    """The attention of QuantAttnBlock alone, fp16 projections as the route hands them over: the library passes (bmm, * scale,
    softmax, bmm on fp32, as the route's fallback runs them) against qd_attn_h16."""
    import torch.nn.functional as F
    from qdiff import engine
    prev = engine.WEIGHT_ONLY_ATTN
    engine.set_weight_only_attention(torch.float16)
    g = torch.Generator(device=dev).manual_seed(0)
    try:
        for B, T, d in shapes:
            q, k, v = (torch.randn(B, T, d, device=dev, generator=g) for _ in range(3))
            qh, kh, vh = q.half(), k.half(), v.half()
            st = (T * d, d, d, 1)
            scale = d ** -0.5
            lib = 1000 * _events_ms(lambda: torch.bmm(F.softmax(torch.bmm(q, k.transpose(1, 2)) * scale, dim=2), v))
            us = 1000 * _events_ms(lambda: engine.attention_h16(qh, kh, vh, B, T, T, 1, d, st, st, st, scale, torch.float16))
            print(json.dumps({"B": B, "T": T, "d": d, "library_fp32_us": round(lib, 1), "kernel_us": round(us, 1),
                              "tflops": round(4.0 * B * T * T * d / us / 1e6, 1), "speedup_vs_library": round(lib / us, 2)}), flush=True)
    finally:
        engine.set_weight_only_attention(prev)


# LSUN-Churches LDM-8 at batch 16: (H = W, channels) of the maps its residual blocks normalise
CHURCHES_GN_SHAPES = [(32, 192), (32, 384), (16, 384), (16, 768), (8, 384), (8, 768), (4, 768), (4, 1536), (2, 768), (2, 1536)]


def mod_shape_table(dev, B=16):
    """The three launch forms alone against today's passes over the same tensors (library GroupNorm, SiLU, modulation / resampling
    in fp32 NCHW-logical tensors, then qd_rows_to_h16) and a device copy of the bytes the new form moves."""
    import torch.nn.functional as F
    from types import SimpleNamespace as NS
    from qdiff import engine, hip
    g = torch.Generator(device=dev).manual_seed(0)

    def med(fn):
        v = sorted(1000 * _events_ms(fn, 20) for _ in range(3))
        return [round(v[1], 1), round(v[0], 1), round(v[2], 1)]       # median, min, max

    def copy_us(nbytes):
        src = torch.empty(max(nbytes // 2, 16), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        return med(lambda: dst.copy_(src))[0]

    for hw, C in CHURCHES_GN_SHAPES:
        S = hw * hw
        x = torch.randn(B * S, C, device=dev, generator=g)
        xn = x.view(B, hw, hw, C).permute(0, 3, 1, 2)                  # the channels-last NCHW tensor today's path sees
        gn = torch.nn.GroupNorm(32, C).to(dev)
        mod = torch.randn(B, 2 * C, device=dev, generator=g)
        plan = NS(ldx=C, act_dtype=torch.float16, pack=NS(segs=[dict(c0w=0, clen=C, clen_pad=C)]), segs=[dict(c0=0)])
        ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=dev)

        def today(kind):
            h = F.silu(gn(xn)) if kind != "mod" else gn(xn)
            if kind == "mod":
                h = F.silu(h * (1 + mod[:, :C, None, None]) + mod[:, C:, None, None])
            elif kind == "down":
                h = F.avg_pool2d(h, 2)
            elif kind == "up":
                h = F.interpolate(h, scale_factor=2, mode="nearest")
            sb, sc, sh, sw = h.stride()
            if sh != h.shape[3] * sw:
                h = h.contiguous(memory_format=torch.channels_last)
                sb, sc, sh, sw = h.stride()
            return engine.wonly_rows(h, plan, h.shape[0], C, h.shape[2] * h.shape[3], (sb, sc, sw))

        forms = [("mod", lambda: engine.wonly_groupnorm_mod_rows(x, B, S, C, gn, mod, True, plan), B * S * C * 10),
                 ("up", lambda: engine.wonly_groupnorm_resample_rows(x, B, hw, hw, C, gn, True, 2, plan), B * S * C * 16)]
        if hw % 2 == 0:
            forms.append(("down", lambda: engine.wonly_groupnorm_resample_rows(x, B, hw, hw, C, gn, True, 1, plan), B * S * C * 8 + B * S * C // 2))
        with torch.no_grad():
            for kind, fn, nbytes in forms:
                new, old = med(fn), med(lambda: today(kind))
                print(json.dumps({"op": "groupnorm_" + kind + "_h16", "shape": [B, hw, hw, C], "us_med_min_max": new, "today_us_med_min_max": old,
                                  "speedup": round(old[0] / new[0], 2), "gbs": round(nbytes / new[0] / 1e3, 1),
                                  "device_copy_same_bytes_us": copy_us(nbytes)}), flush=True)
        del x, ws


# Under-filled contractions at batch 16: (name, H = W, kernel, input segments, Cout); M = 16 * H * W unless given
SPLITK_SHAPES = [
    ("sd 8x8 3x3 1280->1280", 8, 3, [1280], 1280), ("sd 8x8 3x3 2560->1280 shortcut", 8, 3, [1280, 1280], 1280),
    ("sd 16x16 3x3 1280->1280", 16, 3, [1280], 1280), ("sd 16x16 3x3 640->1280", 16, 3, [640], 1280),
    ("sd 16x16 3x3 2560->1280 shortcut", 16, 3, [1280, 1280], 1280), ("sd 16x16 3x3 1920->1280 shortcut", 16, 3, [1280, 640], 1280),
    ("sd 16x16 1x1 1280->1280", 16, 1, [1280], 1280), ("sd 16x16 ff out 5120->1280", 16, 1, [5120], 1280),
    ("sd 8x8 1x1 2560->1280 skip", 8, 1, [1280, 1280], 1280),
    ("sd 32x32 3x3 640->640", 32, 3, [640], 640), ("sd 32x32 3x3 1920->640 shortcut", 32, 3, [1280, 640], 640),
    ("sd to_k / to_v M=1232 768->1280", (1, 1232), 1, [768], 1280), ("sd to_k / to_v M=1232 768->640", (1, 1232), 1, [768], 640),
    ("sd temb M=16 1280->1280", (1, 16), 1, [1280], 1280),
    ("ldm 8x8 3x3 896->896", 8, 3, [896], 896), ("ldm 8x8 3x3 1792->896 shortcut", 8, 3, [896, 896], 896),
    ("ldm 16x16 3x3 672->672", 16, 3, [672], 672), ("ldm 16x16 3x3 1568->672 shortcut", 16, 3, [896, 672], 672),
    ("ldm 32x32 3x3 448->448", 32, 3, [448], 448),
]


def splitk_shape_table(dev, counts=(2, 3, 4, 6, 8, 12, 16)):
    from types import SimpleNamespace as NS
    from qdiff import engine, hip
    g = torch.Generator(device=dev).manual_seed(0)
    prev = engine.WEIGHT_ONLY_SPLITK
    engine.set_weight_only_splitk(True)

    def quant(w):
        flat = w.reshape(w.shape[0], -1)
        mn, mx = flat.min(1)[0].clamp(max=0), flat.max(1)[0].clamp(min=0)
        d = ((mx - mn) / 15).clamp(min=1e-8)
        return NS(delta=d, zero_point=torch.round(-mn / d), n_bits=4, n_levels=16, sym=False, alpha=None, soft_targets=False)

    def med(fn):
        v = sorted(1000 * _events_ms(fn, 20) for _ in range(3))
        return [round(v[1], 1), round(v[0], 1), round(v[2], 1)]       # median, min, max

    try:
        for name, hw, k, segs, Cout in SPLITK_SHAPES:
            B, H, W = (16, hw, hw) if isinstance(hw, int) else (1,) + hw
            Cin = sum(segs)
            w = torch.randn(Cout, Cin, k, k, device=dev, generator=g) * 0.05
            bounds = [(0, segs[0])] + ([(segs[0], Cin)] if len(segs) == 2 else [])
            pack = engine.pack_module_weights(w if k > 1 else w.view(Cout, Cin, 1, 1), [quant(w[:, a:b]) for a, b in bounds], segs[0] if len(segs) == 2 else 0)
            bias = torch.randn(Cout, device=dev, generator=g)
            for dname, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
                plan = engine.build_wonly_plan(pack, k, k, 1, k // 2, bias, dt)
                M = B * H * W
                xh = torch.randn(M, plan.ldx, device=dev, generator=g).to(dt)
                fn = lambda: engine.wonly_forward(plan, xh, B, H, W, H, W)
                call = hip.ConvCall(x=xh, w=pack.wq, out=bias, ldx=plan.ldx, ldk=pack.ldk, ldo=Cout, B=B, H=H, W=W, Ho=H, Wo=W, Cout=Cout, kh=k, kw=k,
                                    stride=1, pad_t=k // 2, pad_l=k // 2, wbits=pack.wbits, w_tiled=True, segs=plan.segs)
                row = {"layer": name, "operands": dname, "M": M, "N": Cout, "tiles": ((M + 127) // 128) * ((Cout + 127) // 128),
                       "ksteps": k * k * sum((s["clen"] + 63) // 64 for s in plan.segs)}
                hip.wq_h16_config(0)
                row["unsplit_us"] = med(fn)
                for n in counts:
                    hip.wq_h16_config(n)
                    got = hip.wq_h16_splitk_ws_bytes(call) // (M * Cout * 4)
                    if got == n:
                        row[f"n{n}_us"] = med(fn)
                hip.wq_h16_config(-1)
                row["policy_nsplit"] = hip.wq_h16_splitk_ws_bytes(call) // (M * Cout * 4) or 1
                row["policy_us"] = med(fn)
                print(json.dumps(row), flush=True)
            del w, pack, plan, xh
    finally:
        hip.wq_h16_config(-1)
        engine.set_weight_only_splitk(prev)


def wide_shape_table(dev):
    """The GEGLU projection alone at SD's three shapes (W4, fp16): one launch with the GEGLU epilogue on the interleaved pack
    against the linear launch (fp32 [M][2F]) + qd_geglu_h16 on the same weights."""
    from types import SimpleNamespace as NS
    from qdiff import engine, hip
    g = torch.Generator(device=dev).manual_seed(0)
    for M, C in SD_LN_SHAPES:
        Fd = 4 * C
        w = torch.randn(2 * Fd, C, device=dev, generator=g) * 0.05
        flat_min, flat_max = w.min(1)[0].clamp(max=0), w.max(1)[0].clamp(min=0)
        d = ((flat_max - flat_min) / 15).clamp(min=1e-8)
        q = NS(delta=d, zero_point=torch.round(-flat_min / d), n_bits=4, n_levels=16, sym=False, alpha=None, soft_targets=False)
        bias = torch.randn(2 * Fd, device=dev, generator=g)
        pack = engine.pack_module_weights(w, [q], 0)
        plan = engine.build_wonly_plan(pack, 1, 1, 1, 0, bias, torch.float16)
        gplan = engine.build_wonly_plan(engine.pack_select_tiles(pack, engine.geglu_row_perm(Fd, dev)), 1, 1, 1, 0, bias, torch.float16, geglu=True)
        nxt = NS(segs=[dict(c0=0)], pack=NS(segs=[dict(c0w=0, clen=Fd)]), ldx=Fd, act_dtype=torch.float16)   # the FF output's row layout
        xh = torch.randn(M, C, device=dev, generator=g).half()
        o2 = torch.empty(M, Fd, dtype=torch.float16, device=dev)

        def two():
            h = engine.wonly_forward(plan, xh, 1, 1, M, 1, M)
            hip.geglu_h16(h, M, Fd, 2 * Fd, o2, Fd)

        lin = 1000 * _events_ms(lambda: engine.wonly_forward(plan, xh, 1, 1, M, 1, M), 20)
        both = 1000 * _events_ms(two, 20)
        epi = 1000 * _events_ms(lambda: engine.wonly_forward_geglu(gplan, xh, M, nxt), 20)
        print(json.dumps({"op": "geglu_projection", "M": M, "K": C, "F": Fd, "linear_us": round(lin, 1), "linear_plus_geglu_h16_us": round(both, 1),
                          "geglu_epilogue_us": round(epi, 1), "speedup": round(both / epi, 2)}), flush=True)
        del w, pack, plan, gplan, xh, o2


STREAM_CEILING_GBS = 6300.0        # HBM streaming ceiling of element-wise kernels (cdna_hip_programming.md Appendix B)
# SD-v1.4 at batch 16: (tokens M = 16 * H * W, channels C) of the four latent levels; GroupNorm also at the widths of the
# concatenated up-path inputs
SD_LN_SHAPES = [(65536, 320), (16384, 640), (4096, 1280)]
SD_GN_SHAPES = [(16, 4096, 320), (16, 4096, 640), (16, 4096, 960), (16, 1024, 640), (16, 1024, 1280), (16, 1024, 1920), (16, 256, 1280),
                (16, 256, 2560), (16, 64, 1280), (16, 64, 2560)]


def fuse_shape_table(dev):
    from qdiff import hip
    g = torch.Generator(device=dev).manual_seed(0)

    def row(op, shape, fn, nbytes):
        us = 1000 * _events_ms(fn, 20)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        cp = 1000 * _events_ms(lambda: dst.copy_(src), 20)
        print(json.dumps({"op": op, "shape": shape, "us": round(us, 1), "gbs": round(nbytes / us / 1e3, 1),
                          "of_ceiling": round(nbytes / us / 1e3 / STREAM_CEILING_GBS, 3), "device_copy_same_bytes_us": round(cp, 1)}), flush=True)

    for M, C in SD_LN_SHAPES:
        x = torch.randn(M, C, device=dev, generator=g)
        gm, bt = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        out = torch.empty(M, C, dtype=torch.float16, device=dev)
        row("layernorm_h16", [M, C], lambda: hip.layernorm_h16(x, M, C, C, 1e-5, gm, bt, out, C), M * C * 6)
        Fd = 4 * C
        h = torch.randn(M, 2 * Fd, device=dev, generator=g)
        o2 = torch.empty(M, Fd, dtype=torch.float16, device=dev)
        row("geglu_h16", [M, Fd], lambda: hip.geglu_h16(h, M, Fd, 2 * Fd, o2, Fd), M * Fd * 10)
        del h, o2
    for B, S, C in SD_GN_SHAPES:
        x = torch.randn(B * S, C, device=dev, generator=g)
        gm, bt = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        out = torch.empty(B * S, C, dtype=torch.float16, device=dev)
        ws = torch.empty(hip.groupnorm_ws_bytes(B, C, S), dtype=torch.uint8, device=dev)
        # two reads of x (statistics, apply) and one 16-bit write
        row("groupnorm_h16+silu", [B, S, C], lambda: hip.groupnorm_h16(x, B, S, C, C, 32, 1e-5, gm, bt, True, out, C, ws), B * S * C * 10)


# SD-v1.4 at batch 16 (B*H = 128): self-attention at the four latent levels, cross-attention over 77 tokens
SD_SHAPES = [(128, 4096, 4096, 40), (128, 1024, 1024, 80), (128, 256, 256, 160), (128, 64, 64, 160),
             (128, 4096, 77, 40), (128, 1024, 77, 80), (128, 256, 77, 160), (128, 64, 77, 160)]
# the LDM-4 (LSUN-Bedrooms) and LDM-8 (LSUN-Churches) attention shapes at batch 16
LDM_SHAPES = [(224, 1024, 1024, 32), (336, 256, 256, 32), (448, 64, 64, 32),
              (128, 1024, 1024, 24), (128, 256, 256, 48), (128, 64, 64, 48), (128, 16, 16, 96), (128, 4, 4, 96)]


def attn_shape_table(dev, shapes=SD_SHAPES):
    import torch.nn.functional as F
    from qdiff import engine
    prev = engine.WEIGHT_ONLY_ATTN
    engine.set_weight_only_attention(torch.float16)
    g = torch.Generator(device=dev).manual_seed(0)
    try:
        for BH, T, S, d in shapes:
            q, k, v = (torch.randn(1, n, BH, d, device=dev, generator=g) for n in (T, S, S))
            st = lambda n: (n * BH * d, BH * d, d, 1)
            us = 1000 * _events_ms(lambda: engine.attention_h16(q, k, v, 1, T, S, BH, d, st(T), st(S), st(S), d ** -0.5))
            qh, kh, vh = (t.permute(0, 2, 1, 3).reshape(BH, -1, d).half().contiguous() for t in (q, k, v))
            sdpa = 1000 * _events_ms(lambda: F.scaled_dot_product_attention(qh, kh, vh))
            lib = 1000 * _events_ms(_library_core(BH, T, S, d, dev))
            flop = 4.0 * BH * T * S * d
            print(json.dumps({"BH": BH, "T": T, "S": S, "d": d, "kernel_us": round(us, 1),
                              "tflops": round(flop / us / 1e6, 1), "frac_of_peak": round(flop / us / 1e6 / F16_MFMA_PEAK_TFLOPS, 4),
                              "sdpa_fp16_us": round(sdpa, 1), "library_fp32_us": round(lib, 1),
                              "speedup_vs_library": round(lib / us, 2)}), flush=True)
    finally:
        engine.set_weight_only_attention(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="sd,ldm,cifar")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--evals", type=int, default=3)
    ap.add_argument("--attn", action="store_true", help="the attention-knob column (layer kernel at fp16)")
    ap.add_argument("--attn-shapes", action="store_true", help="the per-shape attention table at SD's shapes")
    ap.add_argument("--fuse", action="store_true", help="the block-fusion column (layer kernel at fp16; with --attn the attention kernel too)")
    ap.add_argument("--rounds", type=int, default=3, help="A/B alternations of --fuse")
    ap.add_argument("--fuse-shapes", action="store_true", help="the three producers alone at SD's shapes")
    ap.add_argument("--wide", action="store_true", help="with --fuse: the wide-fusion column (fusion on, wide off / on alternated) and the "
                                                        "GEGLU projection alone at SD's three shapes")
    ap.add_argument("--splitk", action="store_true", help="the split-K column: every other weights-only knob on, split-K off / on alternated")
    ap.add_argument("--splitk-shapes", action="store_true", help="the under-filled contraction shapes alone: unsplit against forced slice counts")
    ap.add_argument("--mod", action="store_true", help="the column of the scale-shift / resampling residual blocks: fusion on, FUSE_MOD off / on alternated")
    ap.add_argument("--mod-shapes", action="store_true", help="the three launch forms of --mod alone at LSUN-Churches' shapes")
    ap.add_argument("--ddim", action="store_true", help="the column of the DDIM (CIFAR) blocks: every other weights-only knob on (the attention "
                                                        "kernel with --attn), FUSE_DDIM off / on alternated")
    ap.add_argument("--ddim-shapes", action="store_true", help="the DDIM attention alone at B = 64, d = 256, T = 256 and 16: library passes "
                                                               "against the kernel")
    ap.add_argument("--graph", action="store_true", help="HIP-graph replay of the weights-only state: every block-level knob on, eager / "
                                                         "replay alternated; with --temb also the one-launch embedding Linears off / on under replay")
    ap.add_argument("--temb", action="store_true", help="the one-launch embedding Linears (WEIGHT_ONLY_TEMB): alone, off / on alternated on the "
                                                        "eager walk; with --graph, off / on under replay")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from qdiff import hip
    hip.load()
    dev = torch.device("cuda:0")
    if a.attn_shapes:
        attn_shape_table(dev, SD_SHAPES + LDM_SHAPES)
    if a.fuse_shapes:
        fuse_shape_table(dev)
    if a.ddim_shapes:
        ddim_shape_table(dev)
    if a.wide and not a.mod and not a.ddim:
        wide_shape_table(dev)
    if a.mod_shapes:
        mod_shape_table(dev)
    if a.splitk_shapes:
        splitk_shape_table(dev)
    for kind in [m for m in a.models.split(",") if m]:           # --models "" = the shape tables alone
        if a.graph or a.temb:
            res = run_graph(kind, a.batch, a.evals, dev, a.attn, (a.temb, ("graph",) if a.graph else ()), a.rounds)
        elif a.ddim:
            res = run_ddim(kind, a.batch, a.evals, dev, a.attn, a.rounds)
        elif a.mod:
            res = run_mod(kind, a.batch, a.evals, dev, a.attn, a.wide, a.rounds)
        elif a.splitk:
            res = run_splitk(kind, a.batch, a.evals, dev, a.rounds)
        elif a.wide:
            res = run_wide(kind, a.batch, a.evals, dev, a.attn, a.rounds)
        elif a.fuse:
            res = run_fuse(kind, a.batch, a.evals, dev, a.attn, a.rounds)
        else:
            res = (run_attn if a.attn else run)(kind, a.batch, a.evals, dev)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
