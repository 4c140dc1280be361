"""Cases and helpers of test_linear_epilogue_gpu.py: the two bodies of the linear epilogues of csrc/igemm_dma.hip.

A block of qd_conv2d_i8 whose rows all exist, whose columns all lie inside Cout and whose rows may be accessed with 16-byte vectors
writes its tile through the full-tile body (straight-line code, compile-time choices); every other block through the generic body.
qd_conv_config's bit 1 (hip.conv_config(generic_epilogue=True)) sends every block through the generic body.  Each case is launched
both ways and compared bit for bit, and the default launch is held against the CPU oracle (oracle/quant_ref.py): the fp32 rows
with the comparison and bound of test_random_conv_shapes step 3 (2e-5 of the range + 1e-6: conv_tall_tile_cases.within_oracle_bound),
the int32 accumulators exactly (R.int_conv_exact).

Shapes are the smallest that put both kinds of block into one launch: M = 136 rows (one sample of 8 x 17 pixels: a full 128-row
block and a ragged one), one K-step (Cin = 64, 1 x 1: always the four-wave block) or nine (3 x 3: two K-groups unless switched
off), Cout = 320 (full column blocks), 300 (the last 32-column tile is partial) and 318 (Cout % 4 != 0: no vectors at all).  Rows
for GroupNorm partials are samples of 128 (8 x 16), for the periodic residual samples of 48 rows (period shorter than a tile) and
200 rows (a tile straddles the period).  The launch form of every launch is asserted against tests/abi_emulator.py's statement of
the tile policy, which follows the environment thresholds other test files set for the process."""
import contextlib
from types import SimpleNamespace as NS

import torch

import abi_emulator
import conv_tall_tile_cases as T
from oracle import quant_ref as R

F32, F16 = torch.float32, torch.float16


def case(name, N, k, wbits, B=1, hw=(8, 17), dt=F32, rb=False, res=None, gn=False, ldo=None, kgs=(1,), period=0):
    """res: None / "full"; period: rows of the residual (0 = one per output row); ldo: row stride of the output buffer in elements
    (None = Cout); kgs: the qd_conv_config K-group states to run (1 = two K-groups where the launcher wants them, 0 = never)."""
    return NS(name=name, N=N, k=k, wbits=wbits, B=B, hw=hw, dt=dt, rb=rb, res=res, gn=gn, ldo=ldo, kgs=kgs, period=period)


CASES = []
for wb in (4, 8):
    for k in (1, 3):
        kgs = (1, 0) if k == 3 else (1,)
        w = f"w{wb}_k{k}"
        CASES += [
            case(f"{w}_n320_plain", 320, k, wb, kgs=kgs),
            case(f"{w}_n320_rowbias", 320, k, wb, rb=True, kgs=kgs),
            case(f"{w}_n320_residual", 320, k, wb, res="full", kgs=kgs),
            case(f"{w}_n320_rowbias_residual", 320, k, wb, rb=True, res="full"),        # both row operands: the generic body by design
            case(f"{w}_n300_partial_tile_residual", 300, k, wb, res="full"),
            case(f"{w}_n318_no_vectors_rowbias", 318, k, wb, rb=True),
            case(f"{w}_n320_ldo_defeats_vec", 320, k, wb, res="full", ldo=322),
            case(f"{w}_n320_period48", 320, k, wb, B=4, hw=(6, 8), res="full", period=48, kgs=kgs),
            case(f"{w}_n320_period200_straddles", 320, k, wb, B=2, hw=(10, 20), res="full", period=200),
            case(f"{w}_n320_gn", 320, k, wb, B=2, hw=(8, 16), gn=True, kgs=kgs),
            case(f"{w}_n320_gn_rowbias", 320, k, wb, B=2, hw=(8, 16), gn=True, rb=True, kgs=kgs),
            case(f"{w}_n300_gn_residual", 300, k, wb, B=2, hw=(8, 16), gn=True, res="full"),
            case(f"{w}_n320_gn_period128", 320, k, wb, B=2, hw=(8, 16), gn=True, res="full", period=128),
            # fp16 rows on 4-element vectors (a row stride that is no multiple of 8 keeps them off the full-line form)
            case(f"{w}_n320_f16_residual", 320, k, wb, dt=F16, res="full", ldo=324, kgs=kgs),
            case(f"{w}_n320_f16_rowbias_gn", 320, k, wb, B=2, hw=(8, 16), dt=F16, rb=True, gn=True, ldo=324),
        ]


@contextlib.contextmanager
def launches(kgroups):
    """[(form the library answers, form the written-down tile policy gives)] of every hip.conv2d_i8 launch made inside."""
    from qdiff import hip
    seen, real = [], hip.conv2d_i8

    def spy(c, acc_out=None):
        if acc_out is None:
            seen.append((hip.conv2d_i8_form(c), abi_emulator.conv2d_i8_form(c, kgroups=kgroups)))
        return real(c, acc_out=acc_out)
    hip.conv2d_i8 = spy
    try:
        yield seen
    finally:
        hip.conv2d_i8 = real


def build(cuda, c):
    t = T.build(cuda, T.case(c.name, c.N, c.B, c.hw, wbits=c.wbits, Cin=64, k=c.k, dt=c.dt))
    if c.period:
        t.residual[c.period:] = t.residual[:c.period].repeat(t.M // c.period - 1, 1)
        t.residual_cpu[c.period:] = t.residual_cpu[:c.period].repeat(t.M // c.period - 1, 1)
    return t


def run(t, c, kgroups, generic, dt=None):
    """One launch of the case on all rows; returns (rows, GroupNorm partials or None, form)."""
    from qdiff import engine, hip
    dt = c.dt if dt is None else dt
    out = None
    if c.ldo is not None:
        wide = torch.full((t.M, c.ldo), -7.5, dtype=dt, device=t.xq.device)
        out = wide[:, :c.N]
    res = None
    if c.res:
        res = (t.residual[:c.period] if c.period else t.residual).to(dt)
    hip.conv_config(kgroups=kgroups, generic_epilogue=generic)
    try:
        with launches(kgroups) as seen:
            got = engine.conv_forward(t.plan, t.xq, c.B, t.H, t.W, out=out, rowbias=t.rowbias if c.rb else None, residual=res,
                                      out_dtype=dt, splitk=False, gn_stats=c.gn, res_period=c.period)
        torch.cuda.synchronize()
    finally:
        hip.conv_config(kgroups=1)
    assert len(seen) == 1 and seen[0][0] == seen[0][1], f"launch form {seen}: not the form the tile policy states"
    form = seen[0][0]
    assert form[0] == 128 and form[3] == 1, form
    if c.ldo is not None:
        assert bool((wide[:, c.N:] == -7.5).all()), "columns past Cout were written"
    part = getattr(got, "qd_gn_part", None)
    assert (part is not None) == bool(c.gn)
    return got, part, form


def matches_oracle(t, c, out32):
    zero_rb = (lambda b: torch.zeros(1, c.N)) if not c.rb else None
    zero_res = (lambda b: torch.zeros(t.S, c.N)) if not c.res else None
    wrong = {k: f for k, f in (("rowbias", zero_rb), ("residual", zero_res)) if f is not None}
    return T.matches_oracle(t, out32, samples=sorted({0, c.B - 1}), **wrong)


def exact_accumulators(t, c):
    """int32 accumulators with the zero points restored, from the integer oracle: [M][N]."""
    xc = R.uaq_codes(t.x, t.aq.delta, t.z, 8, False)
    want = R.int_conv_exact(xc, int(t.z), t.ly.codes, t.ly.q.zero_point.reshape(-1).long(), "conv2d", dict(stride=1, padding=c.k // 2))
    return want.permute(0, 2, 3, 1).reshape(t.M, c.N)
