"""Shared by the tests of qd_vq_lookup (tests/test_vq_lookup_gpu.py, test_vq_lookup_exact_gpu.py, test_vq_lookup_host.py): the
fp64 margin reference, the byte-checked call, inputs whose scores are EXACT in fp32, and the layouts a latent can arrive in.

Lattice inputs.  z = kz / 16 and codebook = ke / 16 with integers kz, ke in [-127, 127] (wide), or z = kz, codebook = ke with
kz, ke in [-2, 2] (narrow).  Every product z_c e_jc is a multiple of 2^-8, h_j = |e_j|^2 / 2 a multiple of 2^-9, and every partial
sum of the kernel's chain s = h_j; s = fma(-z_c, e_jc, s) an integer number of 2^-9 units below 8 * 127^2 * 2 < 2^18 units at
e_dim <= 8: all of them fp32 numbers (24 bits), all inputs fp16 and bf16 numbers (7 bits and a sign).  So the kernel's score IS
the mathematical score (|e_j|^2 - 2 z.e_j) / 2, and the index of every pixel, ties included, is the first index of the integer
minimum of |ke|^2 - 2 kz.ke: no tolerance, no mask (first_min)."""
import torch

TILE, STAGE, MIN_SLICE, MAX_SLICES = 1024, 512, 128, 64          # include/qdiff_hip.h, the launch form of qd_vq_lookup
FORCED = [-1, 1, 2, 1 << 20]                                     # the rule, one slice, two, the most the rule allows
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
LAYOUTS = ["nchw", "cl", "row", "px", "chslice", "bstride", "offset", "hstride"]
FILL = 77.0                                                      # what surrounds a view: a wrong address reads it


def _margins(z, cb):
    """fp64 on the CPU: (argmin, per-pixel tolerance function of the kernel's index, mask of pixels whose runner-up is farther
    than the tolerance at the minimiser, NaN-pixel mask) for z [B, E, H, W] (already in the kernel's input type)"""
    zr, e = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).double().cpu(), cb.double().cpu()
    d = sum((zr[:, c:c + 1] - e[None, :, c]) ** 2 for c in range(e.shape[1]))
    m = 0.5 * (e ** 2).sum(1)[None] + zr.abs() @ e.abs().t()
    n = e.shape[1] + 3
    gamma = n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
    return d, m, gamma, torch.isnan(zr).any(1)


def _assert_nearest(z, cb, idx):
    d, m, gamma, nan = _margins(z, cb)
    idx = idx.cpu().long()
    assert ((idx >= 0) & (idx < cb.shape[0])).all() and (idx[nan] == 0).all()
    ok = ~nan
    d, m, idx = d[ok], m[ok], idx[ok]
    j0 = d.argmin(1)
    rows = torch.arange(d.shape[0])
    tol = 4 * gamma * torch.maximum(m[rows, idx], m[rows, j0])
    excess = d[rows, idx] - d[rows, j0]
    print(f"worst excess / tol {(excess / tol.clamp_min(1e-300)).max().item() if len(rows) else 0:.3f}")
    assert (excess <= tol).all()
    if d.shape[1] > 1:                                           # determined pixels: the index IS the fp64 argmin
        second = d.topk(2, dim=1, largest=False).values[:, 1]
        det = second - d[rows, j0] > tol
        assert torch.equal(idx[det], j0[det]) and det.any()


def _run(lib, cuda, z, cb, table, out_dtype, ldo, slices):
    """one call with `slices` forced, poisoned workspace, sentinel row: (indices, out rows) after the byte-level checks"""
    from qdiff import hip
    P, T = z.shape[0] * z.shape[2] * z.shape[3], (cb if table is None else table).shape[1]
    lib.qd_vq_config(slices)
    ws = torch.full((max(int(lib.qd_vq_lookup_ws_bytes(z.shape[0], z.shape[2] * z.shape[3], cb.shape[0])), 8),), 255, dtype=torch.uint8, device=cuda)
    buf = torch.full((P + 1, ldo), -1234.0, dtype=out_dtype, device=cuda)
    idx = torch.full((P + 1,), -7, dtype=torch.int32, device=cuda)
    hip.vq_lookup(z, cb, table=table, indices=idx, out=buf[:P], ws=ws)
    torch.cuda.synchronize()
    assert (buf[P] == -1234.0).all() and idx[P].item() == -7    # the row past B*S is not touched
    want = (cb if table is None else table)[idx[:P].long()]
    assert torch.equal(buf[:P, :T], want.to(out_dtype))          # bit for bit in fp32, ONE nearest-even rounding otherwise
    assert (buf[:P, T:] == 0).all()
    return idx[:P].clone()


# ---- inputs whose scores are exact in fp32 -----------------------------------------------------------------------------------
def lattice(kind, n, E, g):
    """int64 [n, E] of the wide ([-127, 127], values k / 16) or narrow ([-2, 2], values k) lattice"""
    r = {"wide": 127, "narrow": 2}[kind]
    return torch.randint(-r, r + 1, (n, E), generator=g, dtype=torch.int64)


def codes(kind, n_e, E, g):
    """int64 [n_e, E] codebook on the lattice.  narrow: n_e draws out of n_e / 3 lattice rows, so that most rows have a duplicate
    at every e_dim (5^E distinct narrow rows are far more than 8192 from e_dim 6 on) and most pixels several exact minimisers"""
    if kind == "wide":
        return lattice(kind, n_e, E, g)
    base = lattice(kind, max(1, n_e // 3), E, g)
    return base[torch.randint(0, base.shape[0], (n_e,), generator=g)]


def values(kind, k):
    """the fp32 values of lattice integers (exact; equally exact after a cast to fp16 or bf16)"""
    return k.float() / 16 if kind == "wide" else k.float()


def distinct_codes(n_e, E):
    """int64 [n_e, E], rows pairwise distinct: the base-b digits of the row index, least significant first, centred; values
    k / 16 (the wide lattice).  b: the smallest base with b^E >= n_e; needs b <= 255."""
    b = 2
    while b ** E < n_e:
        b += 1
    assert b <= 255, f"{n_e} distinct rows of {E} channels need base {b} > 255"
    j = torch.arange(n_e, dtype=torch.int64)
    return torch.stack([(j // b ** c) % b - b // 2 for c in range(E)], dim=1)


def first_min(kz, ke, counts=False):
    """int64 on the CPU: per row of kz [P, E] the FIRST index of the minimum of |ke_j|^2 - 2 kz.ke_j over the rows of ke
    [n_e, E] (twice the kernel's score in units of the lattice step squared); counts=True: also the number of minimisers"""
    kz, ke = kz.long().cpu(), ke.long().cpu()
    n_e = ke.shape[0]
    assert n_e <= 1 << 20 and kz.abs().max() <= 127 and ke.abs().max() <= 127       # the key below stays inside int64
    e2, j = (ke * ke).sum(1), torch.arange(n_e, dtype=torch.int64)
    first, many = [], []
    for rows in kz.split(512):
        s = e2[None] - 2 * (rows @ ke.t())
        key = (s << 20) + j[None]                                 # ordered by (score, index): its minimum is the first minimum
        first.append(key.amin(1) & ((1 << 20) - 1))
        many.append((s == s.amin(1, keepdim=True)).sum(1))
    return (torch.cat(first), torch.cat(many)) if counts else torch.cat(first)


# ---- the layouts a latent can arrive in --------------------------------------------------------------------------------------
def split_pixels(P):
    """(B, H, W) with B * H * W = P: the largest batch of 7, 3, 1 and the largest height of 11, 7, 5, 3, 1 that divide"""
    B = next(b for b in (7, 3, 1) if P % b == 0)
    H = next(h for h in (11, 7, 5, 3, 1) if (P // B) % h == 0 and P // B > h) if P // B > 1 else 1
    return B, H, P // B // H


def place(rows, B, H, W, layout, device):
    """z [B', E, H', W'] on `device` whose pixels, in the kernel's order (batch, then height, then width), are the rows of `rows`
    [B*H*W, E] (any float type), stored as `layout` says.  Views are cut out of storage filled with FILL."""
    P, E = rows.shape
    assert P == B * H * W
    nchw = rows.view(B, H, W, E).permute(0, 3, 1, 2).contiguous().to(device)

    def filled(*shape):
        return torch.full(shape, FILL, dtype=rows.dtype, device=device)

    if layout == "nchw":                                         # strides (E S, S, W, 1): what the sampler hands over
        return nchw
    if layout == "cl":                                           # strides (S E, 1, W E, E)
        return rows.contiguous().to(device).view(B, H, W, E).permute(0, 3, 1, 2)
    if layout == "row":
        return rows.t().contiguous().view(1, E, 1, P).to(device)
    if layout == "px":                                           # S = 1: the batch stride alone walks the pixels
        return rows.contiguous().view(P, E, 1, 1).to(device)
    if layout == "chslice":                                      # channels 2 .. 2+E of a tensor of E + 5
        v = filled(B, E + 5, H, W)[:, 2:2 + E]
    elif layout == "bstride":                                    # every second image of a batch of 2 B
        v = filled(2 * B, E, H, W)[::2]
    elif layout == "offset":                                     # dense, 7 elements into its storage
        v = filled(P * E + 7)[7:].view(B, E, H, W)
    elif layout == "hstride":                                    # rows of W + 3: with H > 1 the two pixel axes do not collapse
        v = filled(B, E, H, W + 3)[..., :W]
    else:
        raise ValueError(layout)
    v.copy_(nchw)
    return v


def pixel_rows(z):
    """[B*H*W, E] in the kernel's pixel order: the inverse of place()"""
    return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
