#!/usr/bin/env python3
"""Output bytes of the epilogue bodies of csrc/igemm_dma.hip from two builds of the library, compared byte for byte.

    python tools/igemm_epilogue_bits.py <parent's libqdiff_hip.so> [<this tree's .so>]  > profiles/igemm_epilogue_bits.txt

Every launch below runs once per library (QDIFF_HIP_LIB), each side in a fresh child process under its own time limit; the run
stops at the first child that does not exit normally.  Inputs come from the case builders of the test suite
(tests/linear_epilogue_cases.py, tests/conv_tall_tile_cases.py) with their fixed seeds, so both sides contract the same operands.
Per launch one line: every output buffer (rows, GroupNorm partials, hd_sum, int32 accumulators) `equal` or its first differing byte.
Exit status 1 on any difference."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "q-diffusion_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CHILD_SECONDS = 240


def child(path):
    import torch
    import torch.nn.functional as F
    import conv_tall_tile_cases as T
    import linear_epilogue_cases as L
    from oracle import quant_ref as R
    from qdiff import engine, hip
    cuda = torch.device("cuda:0")
    hip.load()
    rec = []                                     # [(launch, [(buffer, bytes)])]

    def keep(name, **bufs):
        torch.cuda.synchronize()
        assert all(v is None or bool(v.min() != v.max()) for v in bufs.values()), f"{name}: a buffer the launch left constant"
        rec.append((name, [(k, v.detach().contiguous().cpu().reshape(-1).view(torch.uint8)) for k, v in bufs.items() if v is not None]))

    def linear(c, generics=(False, True)):
        t = L.build(cuda, c)
        for kg in c.kgs:
            for generic in generics:
                rows, part, form = L.run(t, c, kg, generic)
                keep(f"linear {c.name} kgroups={kg} generic={int(generic)} form={form}", rows=rows, gn_part=part)
        return t

    # ---- linear epilogues: single() / full(), both K-group states, the generic body off and on
    for c in L.CASES:
        linear(c)
    # ---- fp16 rows on the full-line form, pair(): ldo = Cout = 320; the row bias per tile (Ho*Wo = 128) and per row (136)
    for k, kgs in ((1, (1,)), (3, (1, 0))):
        for c in (L.case(f"pair_k{k}_residual", 320, k, 4, dt=L.F16, res="full", kgs=kgs),
                  L.case(f"pair_k{k}_rowbias_hw128", 320, k, 4, B=2, hw=(8, 16), dt=L.F16, rb=True, kgs=kgs),
                  L.case(f"pair_k{k}_rowbias_hw136", 320, k, 4, dt=L.F16, rb=True, kgs=kgs),
                  L.case(f"pair_k{k}_gn_residual_hw128", 320, k, 4, B=2, hw=(8, 16), dt=L.F16, res="full", gn=True, kgs=kgs)):
            linear(c, generics=(False,))
    # ---- int32 accumulators (qd_conv2d_i8_acc) and split-K partials + finalise, through both bodies
    for N, k, wbits in ((320, 1, 4), (320, 3, 4), (300, 3, 4), (320, 1, 8), (300, 3, 8)):
        c = L.case(f"acc_n{N}_k{k}_w{wbits}", N, k, wbits)
        t = L.build(cuda, c)
        for generic in (False, True):
            hip.conv_config(kgroups=1, generic_epilogue=generic)
            acc = torch.zeros((t.M, N), dtype=torch.int32, device=cuda)
            engine.conv_forward(t.plan, t.xq, c.B, t.H, t.W, acc_out=acc)
            keep(f"acc {c.name} generic={int(generic)}", acc=acc)
    for wbits in (4, 8):
        c = L.case(f"splitk_w{wbits}", 320, 3, wbits, res="full")
        t = L.build(cuda, c)
        for generic in (False, True):
            hip.conv_config(kgroups=1, generic_epilogue=generic)
            with T.launch_forms() as forms:
                rows = engine.conv_forward(t.plan, t.xq, c.B, t.H, t.W, residual=t.residual, out_dtype=L.F32)
            assert len(forms) == 1 and forms[0][3] >= 2, forms
            keep(f"split-K {c.name} generic={int(generic)} form={forms[0]}", rows=rows)
    # ---- two segments (the 1 x 1 split shortcut of test_two_segments_through_both_bodies)
    for wbits in (4, 8):
        g = torch.Generator().manual_seed(17 + wbits)
        B, C, H, W, Cout, split = 1, 128, 8, 17, 320, 64
        x = F.silu(torch.randn(B, C, H, W, generator=g))
        x[:, split:] *= 3.0
        w = torch.randn(Cout, C, 1, 1, generator=g) * 0.05
        bias = torch.randn(Cout, generator=g)
        qs, aqs = [], []
        for ws in (w[:, :split], w[:, split:]):
            delta, zp = R.uaq_init_scale(ws, wbits, False, True, "max")
            qs.append(T.NS(delta=delta, zero_point=zp, n_bits=wbits, sym=False, n_levels=2 ** wbits, alpha=torch.rand(ws.shape, generator=g) - 0.5,
                           soft_targets=False))
        for xs in (x[:, :split], x[:, split:]):
            d, z = R.uaq_init_scale(xs, 8, False, False, "max")
            aqs.append(T.NS(delta=torch.tensor(float(d)), zero_point=z, n_bits=8, sym=False))
        plan = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), qs, split), aqs, 1, 1, 1, 0, bias.to(cuda))
        xq = engine.quantize_rows(x.to(cuda), plan, B, C, H * W, (C * H * W, H * W, 1))
        res = torch.randn(B * H * W, Cout, generator=g).to(cuda)
        for dt in (L.F32, L.F16):
            for generic in (False, True):
                hip.conv_config(kgroups=1, generic_epilogue=generic)
                with T.launch_forms() as forms:
                    rows = engine.conv_forward(plan, xq, B, H, W, residual=res.to(dt), out_dtype=dt, splitk=False)
                keep(f"two segments w{wbits} {str(dt)[6:]} generic={int(generic)} form={forms[0]}", rows=rows)
    hip.conv_config(kgroups=1)

    # ---- int8 epilogues: head rows (O_HROWS: tile2 at d = 40, tile1 at d = 36), transposed head rows (O_HTR), GEGLU
    grid = engine.act_grid(8, False)
    qp = hip.make_qparams(torch.tensor(0.02, device=cuda), torch.tensor(131.0, device=cuda))
    Bh, Tk, Hh = 2, 128, 8
    for d in (40, 36):
        N = Hh * d
        t = T.build(cuda, T.case(f"heads_d{d}", N, Bh, (8, 16), Cin=64, k=1))
        pl = t.plan

        def heads_call(out8, residual=None, hsum=None):
            return hip.ConvCall(x=t.xq, w=pl.pack.wq, out=out8, bias=pl.bias, residual=residual, ldx=pl.ldx, ldk=pl.pack.ldk, ldo=0,
                                ldr=0 if residual is None else residual.stride(0), B=Bh, H=1, W=Tk, Ho=1, Wo=Tk, Cout=N, kh=1, kw=1,
                                stride=1, pad_t=0, pad_l=0, wbits=pl.pack.wbits, w_tiled=True, segs=pl.segs,
                                epilogue=hip.EPI_HEADS_T_I8 if hsum is not None else hip.EPI_HEADS_I8, oq_params=qp, oq_grid=grid,
                                heads=dict(H=Hh, d=d, T=Tk, Tpad=160, dpad=64, prescale=0.4, sum=hsum))
        for res in (None, L.F32, L.F16):
            q8 = torch.full((Bh * Hh, 160, 64), 77, dtype=torch.int8, device=cuda)
            call = heads_call(q8, None if res is None else t.residual.to(res))
            form = hip.conv2d_i8_form(call)
            hip.conv2d_i8(call)
            keep(f"head rows d={d} residual={'none' if res is None else str(res)[6:]} form={form}", rows=q8)
        v8 = torch.full((Bh * Hh, 64, 160), 77, dtype=torch.int8, device=cuda)
        hs = torch.zeros((Bh * Hh, 64), dtype=torch.int32, device=cuda)
        call = heads_call(v8, hsum=hs)
        form = hip.conv2d_i8_form(call)
        hip.conv2d_i8(call)
        keep(f"transposed head rows d={d} form={form}", rows=v8, hd_sum=hs)
    M, K, Fd = 136, 64, 320
    g = torch.Generator().manual_seed(640)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(2 * Fd, K, generator=g) * 0.05
    delta, zp = R.uaq_init_scale(w, 4, False, True, "max")
    q = T.NS(delta=delta, zero_point=zp, n_bits=4, sym=False, n_levels=16, alpha=torch.rand(w.shape, generator=g) - 0.5, soft_targets=False)
    dx, zx = R.uaq_init_scale(x, 8, False, False, "max")
    aq = T.NS(delta=torch.tensor(float(dx)), zero_point=zx, n_bits=8, sym=False)
    pl = engine.build_conv_plan(engine.pack_module_weights(w.to(cuda), [q], 0, row_perm=engine.geglu_row_perm(Fd, cuda)), [aq], 1, 1, 1, 0,
                                torch.randn(2 * Fd, generator=g).to(cuda))
    xq = engine.quantize_rows(x.to(cuda), pl, 1, K, M, (0, 1, K))
    out8 = torch.full((M, Fd), 77, dtype=torch.int8, device=cuda)
    call = hip.ConvCall(x=xq, w=pl.pack.wq, out=out8, bias=pl.bias, ldx=pl.ldx, ldk=pl.pack.ldk, ldo=Fd, B=1, H=1, W=M, Ho=1, Wo=M,
                        Cout=2 * Fd, kh=1, kw=1, stride=1, pad_t=0, pad_l=0, wbits=4, w_tiled=True, segs=pl.segs,
                        epilogue=hip.EPI_GEGLU_I8, oq_params=qp, oq_grid=grid)
    form = hip.conv2d_i8_form(call)
    hip.conv2d_i8(call)
    keep(f"GEGLU M={M} Cout={2 * Fd} form={form}", rows=out8)

    # ---- the 16-bit float mode (qd_conv2d_bf16): bf16 (wbits 16) and fp16 (17) operands, a residual and GroupNorm partials
    for dt in (torch.bfloat16, torch.float16):
        for Cout in (128, 100):
            g = torch.Generator().manual_seed(1600 + Cout)
            Bc, Hc, Wc, Cin = 1, 8, 16, 16
            xr = torch.randn(Bc * Hc * Wc, Cin, generator=g).to(cuda).to(dt)
            wt = hip.pack_weights_bf16((torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1).to(cuda), dt)
            bias = torch.randn(Cout, generator=g).to(cuda)
            res = torch.randn(Bc * Hc * Wc, Cout, generator=g).to(cuda)
            for odt in (torch.float32, dt):
                out = torch.full((Bc * Hc * Wc, Cout), -7.5, dtype=odt, device=cuda)
                part = torch.zeros((Bc, 1, Cout, 2), dtype=torch.float32, device=cuda)
                hip.conv2d_bf16(xr, wt, bias, out, Bc, Hc, Wc, Cin, Cout, k=3, pad=1, residual=res.to(odt), gn_part=part)
                keep(f"qd_conv2d_bf16 wbits={17 if dt == torch.float16 else 16} Cout={Cout} out={str(odt)[6:]}", rows=out, gn_part=part)
    torch.save(rec, path)


def main():
    libs = [os.path.abspath(a) for a in sys.argv[1:3]]
    if len(libs) == 1:
        libs.append(os.path.join(ROOT, "q-diffusion_amd", "lib", "libqdiff_hip.so"))
    import torch
    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):
            path = os.path.join(tmp, f"side{i}.pt")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=dict(os.environ, QDIFF_HIP_LIB=lib),
                                   timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired:
                print(f"{lib}: no result within {CHILD_SECONDS} s; stopped")
                return 2
            if r.returncode != 0:
                print(f"{lib}: child exited with status {r.returncode}; stopped")
                return 2
            sides.append(torch.load(path))
    a, b = sides
    assert [n for n, _ in a] == [n for n, _ in b], "the two sides ran different launches"
    print("launch | output buffers (parent library vs this tree), each 'equal' or first differing byte")
    width = max(len(n) for n, _ in a) + 2
    bad = 0
    for (name, ba), (_, bb) in zip(a, b):
        cells = []
        for (k, va), (_, vb) in zip(ba, bb):
            if va.numel() == vb.numel() and torch.equal(va, vb):
                cells.append(f"{k} equal")
            else:
                bad += 1
                ne = (va[:min(va.numel(), vb.numel())] != vb[:min(va.numel(), vb.numel())]).nonzero()
                cells.append(f"{k} DIFFERS at byte {int(ne[0]) if len(ne) else min(va.numel(), vb.numel())} of {va.numel()}")
        print(f"{name:{width}s}{', '.join(cells)}")
    print(f"{len(a)} launches, {sum(len(x) for _, x in a)} buffers, {bad} differing")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main())
