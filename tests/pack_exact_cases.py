"""Cases of test_pack_exact_host.py / test_pack_exact_gpu.py: the tile-ordered weight packers qd_pack_weights_t4 / _t8
(csrc/igemm_dma.hip) held to the exact bytes, sums and decoded values at the edges.  CPU only, deterministic.

TEST INFRASTRUCTURE.  A case is one weight tensor, one or two channel segments with their own quantiser, the calls that pack them
into ONE buffer, and what that buffer and `wsum` must hold afterwards:

  * codes: oracle.quant_ref.nearest_codes / adaround_codes — torch CPU fp32 with IEEE division, as the reference computes them
    (a quotient in higher precision is a DIFFERENT function on the near-integer family, see reciprocal_changes);
  * layout: include/qdiff_hip.h restated as a plain index formula (expected_image), deliberately without the permutes of
    tests/abi_emulator.py, so that the emulator is held to the formula as the kernels are.

Element (n, t, c) of a segment with nst = ceil(pad16(clen) / 64), ntiles = ceil(Cout / 32):
    kstep = kstep0 + t * nst + c // 64, jt = n // 32, nn = n % 32, kh4 = (c % 64) // 16, j = c % 16
    t8: byte (kstep * ntiles + jt) * 2048 + (kh4 * 32 + nn) * 16 + j holds (code - 128) & 0xff
    t4: the 8-byte unit at (kstep * ntiles + jt) * 1024 + (kh4 * 32 + nn) * 8; code j is the low nibble of byte j (j < 4), the high
        nibble of byte j - 4 (j < 8), the low nibble of byte j - 4 (j < 12), the high nibble of byte j - 8 (j < 16)
Every other byte of the K-steps [kstep0, kstep0 + taps * nst) is 0; every byte outside keeps the sentinel 0xA5 (the buffer has one
spare K-step on each side).  wsum[n] = initial + sum of code (t4) / of code - 128 (t8) over the real elements.
"""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import quant_ref as R

SENTINEL = 0xA5
TILE_BYTES = {4: 1024, 8: 2048}


def pad16(n):
    return (n + 15) // 16 * 16


def zero_points(L):
    """The zero points at the limits engine.pack_module_weights accepts (-128 ... 255) and at the ends of the grid."""
    return [-128, -1, 0, L - 1, L, 255]


def nsteps(clen):
    return (pad16(clen) + 63) // 64


# ------------------------------------------------------------------------------------------------
# expectation
# ------------------------------------------------------------------------------------------------
def seg_codes(c, s):
    """int64 [Cout][clen][taps]: the reference's codes of segment s."""
    wv = c.w.reshape(c.Cout, c.Cin_total, c.taps)[:, s.c0:s.c0 + s.clen]
    d, z = s.delta.view(-1, 1, 1), s.zp.view(-1, 1, 1)
    if s.alpha is not None:
        return R.adaround_codes(wv, d, z, s.alpha, c.n_levels)
    return R.nearest_codes(wv, d, z, c.n_levels)


def element_address(c, s):
    """(byte address, shift) int64 arrays [Cout][clen][taps] of every real element of segment s: the index formula above."""
    ntiles = (c.Cout + 31) // 32
    nst = nsteps(s.clen)
    n, ch, t = np.meshgrid(np.arange(c.Cout), np.arange(s.clen), np.arange(c.taps), indexing="ij")
    kstep = s.kstep0 + t * nst + ch // 64
    jt, nn, kh4, j = n // 32, n % 32, (ch % 64) // 16, ch % 16
    if c.bits == 8:
        return (kstep * ntiles + jt) * 2048 + (kh4 * 32 + nn) * 16 + j, np.zeros_like(j)
    byte = np.where(j < 4, j, np.where(j < 12, j - 4, j - 8))
    shift = np.where((j // 4) % 2 == 1, 4, 0)
    return (kstep * ntiles + jt) * 1024 + (kh4 * 32 + nn) * 8 + byte, shift


def expected_image(c):
    """(uint8 buffer, int64 wsum or None): what the calls of case c leave behind."""
    ntiles = (c.Cout + 31) // 32
    tile = TILE_BYTES[c.bits]
    buf = np.full(c.total_steps * ntiles * tile, SENTINEL, dtype=np.uint8)
    wsum = None if c.wsum0 is None else c.wsum0.numpy().astype(np.int64).copy()
    for s in c.segs:
        codes = seg_codes(c, s).numpy()
        k0, k1 = s.kstep0, s.kstep0 + c.taps * nsteps(s.clen)
        buf[k0 * ntiles * tile:k1 * ntiles * tile] = 0
        addr, shift = element_address(c, s)
        if c.bits == 8:
            buf[addr.ravel()] = ((codes - 128) & 0xff).astype(np.uint8).ravel()
        else:
            assert codes.min() >= 0 and codes.max() <= 15
            for sh in (0, 4):                                  # within one half every address occurs once
                m = shift == sh
                buf[addr[m]] |= (codes[m] << sh).astype(np.uint8)
        if wsum is not None:
            wsum += (codes - (128 if c.bits == 8 else 0)).sum(axis=(1, 2))
    return buf, wsum


def buffer_bytes(c):
    return c.total_steps * ((c.Cout + 31) // 32) * TILE_BYTES[c.bits]


def make_case(name, bits, n_levels, w, segs, Cin_total, taps, wsum0="zero", orders=None, family=""):
    """segs: list of dict(c0, clen, delta [Cout], zp [Cout], alpha [Cout][clen][taps] or None), in buffer order.  wsum0: 'zero', None
    (the packer gets NULL) or an int32 tensor [Cout]."""
    Cout = w.shape[0]
    assert w.dtype == torch.float32 and w.numel() == Cout * Cin_total * taps and not torch.isnan(w).any()
    out, k = [], 1                                             # K-step 0 is the spare one in front
    for s in segs:
        assert s["delta"].shape == (Cout,) and s["zp"].shape == (Cout,) and s["c0"] + s["clen"] <= Cin_total
        assert s["alpha"] is None or s["alpha"].shape == (Cout, s["clen"], taps)
        out.append(NS(c0=s["c0"], clen=s["clen"], kstep0=k, delta=s["delta"].float().contiguous(), zp=s["zp"].float().contiguous(),
                      alpha=None if s["alpha"] is None else s["alpha"].float().contiguous()))
        k += taps * nsteps(s["clen"])
    if isinstance(wsum0, str):
        wsum0 = torch.zeros(Cout, dtype=torch.int32)
    c = NS(name=name, family=family or name.split("_")[0], bits=bits, n_levels=n_levels, w=w.reshape(Cout, Cin_total, taps).contiguous(),
           segs=out, Cin_total=Cin_total, taps=taps, Cout=Cout, wsum0=wsum0, total_steps=k + 1,
           orders=orders or [list(range(len(out)))])
    c.want_buf, c.want_wsum = expected_image(c)
    return c


def run_packers(c, order, t4, t8, dev="cpu"):
    """The calls of case c in `order` through packers with the signature of qdiff.hip.pack_weights_t4 / _t8 (the real ones or
    the emulator's) -> (uint8 numpy buffer, int64 numpy wsum or None)."""
    buf = torch.full((buffer_bytes(c),), SENTINEL, dtype=torch.uint8).to(dev)
    wsum = None if c.wsum0 is None else c.wsum0.clone().to(dev)
    w = c.w.to(dev)
    for i in order:
        s = c.segs[i]
        (t4 if c.bits == 4 else t8)(w, None if s.alpha is None else s.alpha.to(dev), s.delta.to(dev), s.zp.to(dev), c.Cout, c.Cin_total,
                                    c.taps, s.c0, s.clen, c.n_levels, buf, s.kstep0, (c.Cout + 31) // 32, wsum)
    return buf.cpu().numpy(), None if wsum is None else wsum.cpu().numpy().astype(np.int64)


def first_difference(c, buf):
    """Where a byte image departs from the expectation first, in the words of the layout."""
    bad = np.flatnonzero(buf != c.want_buf)
    if bad.size == 0:
        return None
    a = int(bad[0])
    tile = TILE_BYTES[c.bits]
    ntiles = (c.Cout + 31) // 32
    kstep, r = divmod(a, ntiles * tile)
    jt, r = divmod(r, tile)
    unit, byte = divmod(r, tile // 128)
    return (f"{c.name}: {bad.size} bytes differ, first at {a} (kstep {kstep}, tile {jt}, kh4 {unit // 32}, row {jt * 32 + unit % 32}, "
            f"byte {byte}): got 0x{int(buf[a]):02x}, want 0x{int(c.want_buf[a]):02x}")


# ------------------------------------------------------------------------------------------------
# value families: one output channel per variant
# ------------------------------------------------------------------------------------------------
def _pow2(e):
    return torch.tensor(2.0, dtype=torch.float64) ** (-torch.as_tensor(e, dtype=torch.float64))


def _grid_targets(L):
    return torch.arange(-3, L + 3, dtype=torch.float64)       # every code, and both clamps crossed


def _f32(x):
    return x.to(torch.float32)


def grid_case(bits, L, zps, alpha, name, half=0.0, wsum0="zero", family=None):
    """w = (c + half - z) * delta, delta = 2^-e with e varied per channel: exact in fp32.  With alpha, w is shifted by
    -(alpha >= 0) * delta so that floor + (alpha >= 0) lands on the same code c."""
    tg = _grid_targets(L)
    chans = [(z, 2 + i % 7) for i, z in enumerate(zps)]
    Cout, clen = len(chans), tg.numel()
    z = torch.tensor([float(a) for a, _ in chans], dtype=torch.float64)
    d = _pow2([e for _, e in chans])
    al = None
    up = torch.zeros(Cout, clen, dtype=torch.float64)
    if alpha:
        al = torch.where((torch.arange(Cout * clen).view(Cout, clen) * 7 + 3) % 5 < 2, -0.37, 0.41).float().view(Cout, clen, 1)
        up = (al[..., 0] >= 0).double()
    w64 = (tg.view(1, -1) + half - z.view(-1, 1) - up) * d.view(-1, 1)
    w = _f32(w64)
    assert torch.equal(w.double(), w64)
    return make_case(name, bits, L, w.view(Cout, clen, 1), [dict(c0=0, clen=clen, delta=_f32(d), zp=_f32(z), alpha=al)], clen, 1, wsum0, family=family)


ALPHAS = [0.0, -0.0, 1.401298464324817e-45, -1.401298464324817e-45, 1e-30, -1e-30, 10.0, -10.0, math.inf, -math.inf]


def alpha_sign_case(bits, L):
    """One channel per alpha value; w on exact multiples of delta and on the neighbouring fp32 numbers either side of them."""
    Cout = len(ALPHAS)
    ks = torch.arange(-2, min(L, 24) + 2, dtype=torch.float64)
    d = _pow2([3 + i % 4 for i in range(Cout)])
    z = torch.tensor([float((1, 0, 2)[i % 3]) for i in range(Cout)], dtype=torch.float64)
    on = _f32(ks.view(1, -1) * d.view(-1, 1))
    w = torch.stack([on, torch.nextafter(on, torch.full_like(on, math.inf)), torch.nextafter(on, torch.full_like(on, -math.inf))], dim=2)
    w = w.reshape(Cout, -1)
    clen = w.shape[1]
    al = torch.tensor(ALPHAS, dtype=torch.float32).view(-1, 1, 1).expand(Cout, clen, 1).contiguous()
    assert al[2, 0, 0] > 0 and al[2, 0, 0] < 1.2e-38 and math.copysign(1.0, al[1, 0, 0].item()) == -1.0
    return make_case(f"alphasign_t{bits}", bits, L, w.view(Cout, clen, 1), [dict(c0=0, clen=clen, delta=_f32(d), zp=_f32(z), alpha=al)], clen, 1)


def near_integer_weights(L, Cout, seed):
    """Ordinary delta in 0.002 ... 0.012; w = fl(k * delta) and fl((k + 1/2) * delta), k over the grid and a little beyond."""
    g = torch.Generator().manual_seed(seed)
    d = _f32(0.002 + 0.010 * torch.rand(Cout, generator=g, dtype=torch.float64))
    zs = (255, -128, L // 2, 0, L - 1, 3, 200, -77)
    z = torch.tensor([float(zs[i % len(zs)]) for i in range(Cout)])
    ks = torch.arange(-2, L + 2, dtype=torch.float32).view(1, -1) - z.view(-1, 1)
    w = torch.stack([ks * d.view(-1, 1), (ks + 0.5) * d.view(-1, 1)], dim=2).reshape(Cout, -1)      # fp32 products: fl(k * delta)
    return w, d, z


def near_integer_case(bits, L, alpha):
    Cout = 16
    w, d, z = near_integer_weights(L, Cout, 100 + bits)
    clen = w.shape[1]
    al = None
    if alpha:
        al = torch.where((torch.arange(Cout * clen).view(Cout, clen, 1) * 5 + 1) % 3 == 0, 0.25, -0.25).float()
    return make_case(f"nearint_t{bits}_{'alpha' if alpha else 'round'}", bits, L, w.view(Cout, clen, 1),
                     [dict(c0=0, clen=clen, delta=d, zp=z, alpha=al)], clen, 1, family="nearint")


def reciprocal_changes(c):
    """(changed, total): the elements of the case whose code changes when the quotient is computed as w * fl(1 / delta) — from
    the reference's operations alone (what a packer that multiplied by a reciprocal would produce)."""
    changed = total = 0
    for s in c.segs:
        wv = c.w[:, s.c0:s.c0 + s.clen]
        d, z = s.delta.view(-1, 1, 1), s.zp.view(-1, 1, 1)
        q = wv * (1.0 / d)
        q = torch.floor(q) + (s.alpha >= 0).float() if s.alpha is not None else torch.round(q)
        other = torch.clamp(q + z, 0, c.n_levels - 1).to(torch.int64)
        changed += int((other != seg_codes(c, s)).sum())
        total += other.numel()
    return changed, total


def degenerate_case(bits, L, alpha):
    """All-zero channel with delta = 1e-8, w = +-inf, a quotient that overflows to inf, subnormal weights (delta = 2^-126: the
    quotient of a subnormal by the smallest normal number, ties included)."""
    clen = 48
    tiny = 2.0 ** -149
    rows, ds, zs = [], [], []

    def add(vals, d, z):
        rows.append(torch.tensor(vals, dtype=torch.float32).repeat(clen // len(vals) + 1)[:clen])
        ds.append(d)
        zs.append(z)
    add([0.0, -0.0], 1e-8, 3.0)
    add([math.inf, -math.inf, 1.0, -1.0], 0.05, 2.0)
    add([math.inf, -math.inf], 1e-8, 0.0)
    add([3e38, -3e38, 1e30, -1e30, 1.0, -1.0], 1e-8, 5.0)                                  # the quotient overflows
    add([tiny, -tiny, 1e-40, -1e-40, 1e-39, 0.0], 1e-8, 1.0)                               # subnormal weights, quotient ~ 0
    rows.append(torch.arange(-6, clen - 6, dtype=torch.float64).mul(2.0 ** -128).float())  # k / 4 of the smallest normal
    ds.append(2.0 ** -126)
    zs.append(1.0)
    w = torch.stack(rows)
    Cout = w.shape[0]
    al = None
    if alpha:
        al = torch.where(torch.arange(Cout * clen).view(Cout, clen, 1) % 2 == 0, 1.0, -1.0).float()
    return make_case(f"degenerate_t{bits}_{'alpha' if alpha else 'round'}", bits, L, w.view(Cout, clen, 1),
                     [dict(c0=0, clen=clen, delta=torch.tensor(ds, dtype=torch.float32), zp=torch.tensor(zs), alpha=al)], clen, 1, wsum0=None,
                     family="degenerate")


# ------------------------------------------------------------------------------------------------
# geometry families
# ------------------------------------------------------------------------------------------------
COUTS, CLENS, TAPS = (1, 31, 32, 33, 70), (1, 15, 16, 17, 63, 64, 65, 130), (1, 4, 9)


def geometry_weights(L, Cout, Cin, taps, seed, with_alpha):
    """Channels alternate between the grid family (delta a power of two) and the near-integer family (ordinary delta, w =
    fl(k * delta) / fl((k + 1/2) * delta)); the target code of element (n, c, t) walks -3 ... L + 2; z[n] cycles over the edges."""
    g = torch.Generator().manual_seed(seed)
    zl = zero_points(L)
    n = torch.arange(Cout).view(-1, 1, 1)
    ch = torch.arange(Cin).view(1, -1, 1)
    t = torch.arange(taps).view(1, 1, -1)
    z = torch.tensor([float(zl[(i + seed) % len(zl)]) for i in range(Cout)])
    near = ((torch.arange(Cout) + seed) % 2 == 1)
    d = torch.where(near, _f32(0.002 + 0.010 * torch.rand(Cout, generator=g, dtype=torch.float64)), _f32(_pow2((torch.arange(Cout) % 5 + 3).tolist())))
    tgt = ((ch * taps + t + 5 * n) % (L + 6) - 3).float()
    half = torch.where(near.view(-1, 1, 1) & ((ch + t) % 2 == 1), 0.5, 0.0)
    al = None
    up = torch.zeros(Cout, Cin, taps)
    if with_alpha:
        al = torch.where((n * 3 + ch * 5 + t * 7) % 4 < 2, 0.5, -0.5).float()
        up = torch.where(near.view(-1, 1, 1), 0.0, (al >= 0).float())
    w = (tgt + half - z.view(-1, 1, 1) - up) * d.view(-1, 1, 1)                                      # fp32 product
    return w.contiguous(), d, z, al


def geometry_case(bits, L, Cout, clen, taps, idx):
    w, d, z, al = geometry_weights(L, Cout, clen, taps, idx, with_alpha=idx % 2 == 1)
    wsum0 = (None, "zero", (torch.arange(Cout, dtype=torch.int32) * 1000 - 7))[idx % 3]
    return make_case(f"geom_t{bits}_N{Cout}_c{clen}_t{taps}", bits, L, w, [dict(c0=0, clen=clen, delta=d, zp=z, alpha=al)], clen, taps, wsum0,
                     family="geom")


def two_segment_case(bits, L):
    """Cin_total = 64, segments (c0 5, clen 17) and (c0 22, clen 42), each with its own quantiser and an alpha of the slice's
    shape, packed by two calls into one buffer (and one wsum) in both call orders."""
    Cout, Cin, taps = 33, 64, 4
    wa, da, za, aa = geometry_weights(L, Cout, 17, taps, 11, True)
    wb, db, zb, ab = geometry_weights(L, Cout, 42, taps, 12, True)
    g = torch.Generator().manual_seed(5)
    w = torch.randn(Cout, Cin, taps, generator=g)              # the channels no segment covers must not be read into the pack
    w[:, 5:22], w[:, 22:64] = wa, wb
    return make_case(f"twoseg_t{bits}", bits, L, w, [dict(c0=5, clen=17, delta=da, zp=za, alpha=aa), dict(c0=22, clen=42, delta=db, zp=zb, alpha=ab)],
                     Cin, taps, torch.arange(Cout, dtype=torch.int32) * 3 + 1, orders=[[0, 1], [1, 0]])


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> case, in a fixed order."""
    cs = []
    for bits, L in ((4, 16), (8, 256)):
        zl = zero_points(L)
        cs.append(grid_case(bits, L, zl + zl[::-1], False, f"grid_t{bits}"))
        cs.append(grid_case(bits, L, zl + zl[::-1], True, f"grid_t{bits}_alpha", wsum0=torch.arange(12, dtype=torch.int32) - 40000))
        cs.append(grid_case(bits, L, [0, 1, -1, -2, L - 1, L, 254, 255, -128, -127], False, f"ties_t{bits}", half=0.5))
        cs.append(alpha_sign_case(bits, L))
        for alpha in (False, True):
            cs.append(near_integer_case(bits, L, alpha))
            cs.append(degenerate_case(bits, L, alpha))
        cs.append(two_segment_case(bits, L))
    for b in (1, 2, 3, 4):
        cs.append(grid_case(4, 2 ** b, [0, 2 ** b - 1, -1, 1], b % 2 == 0, f"levels_t4_b{b}", family="levels"))
    for b in (4, 5, 6, 7, 8):
        cs.append(grid_case(8, 2 ** b, [0, 2 ** b - 1, -1, 1], b % 2 == 0, f"levels_t8_b{b}", family="levels"))
    idx = 0
    for bits, L in ((4, 16), (8, 256)):
        for Cout in COUTS:
            for clen in CLENS:
                for taps in TAPS:
                    cs.append(geometry_case(bits, L, Cout, clen, taps, idx))
                    idx += 1
    out = {c.name: c for c in cs}
    assert len(out) == len(cs)
    return out


FAMILIES = ("grid", "ties", "alphasign", "nearint", "degenerate", "twoseg", "levels", "geom")


def by_family(fam):
    return [c for c in all_cases().values() if c.family == fam]
