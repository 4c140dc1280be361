"""qdiff.hip.vq_lookup on CPU tensors (no GPU): the arithmetic of csrc/vq_lookup.hip in torch.

Score of code j for a pixel, as the kernel's header states it: h_j = the fp64 sum of e_jc^2 in channel order, halved, rounded ONCE
to fp32; s = h_j; s = fma(-z_c, e_jc, s) for c = 0 .. e_dim-1 in fp32.  A fused multiply-add is evaluated here as the fp64 value
of (-z_c * e_jc) + s rounded to fp32: the product of two fp32 numbers is exact in fp64, the sum carries one fp64 rounding before
the fp32 one, which coincides with the single rounding of the instruction except on double-rounding ties (none on the lattice
inputs of tests/vq_lookup_cases.py, where every value is exact).  The index is the first strict minimum, found from best = +inf,
index 0: a NaN score never wins, so a NaN pixel gives 0.  out rows: table[index] under one rounding to out's type, zero pad."""
import torch

_TYPES = (torch.float32, torch.float16, torch.bfloat16)


def vq_scores(zr, codebook):
    """fp32 [P, n_e]: the kernel's score of every code for pixel rows zr [P, e_dim] (any of the three input types)"""
    e = codebook.double()
    h = torch.zeros(e.shape[0], dtype=torch.float64)
    for c in range(e.shape[1]):
        h = h + e[:, c] * e[:, c]                                 # (exact products of fp32 numbers, summed in channel order)
    s = (0.5 * h).float()[None].expand(zr.shape[0], -1)
    nz = -zr.float().double()
    for c in range(e.shape[1]):
        s = (nz[:, c:c + 1] * e[None, :, c] + s.double()).float()
    return s


def first_strict_min(s):
    """int64 [P]: what `best = inf, idx = 0; for j: if s_j < best: best, idx = s_j, j` leaves in idx"""
    s = torch.where(torch.isnan(s), torch.full_like(s, float("inf")), s)            # NaN loses every comparison
    j = torch.arange(s.shape[1])[None].expand_as(s)
    return torch.where(s == s.amin(1, keepdim=True), j, s.shape[1]).amin(1)         # all +inf: nothing won, index 0


def vq_lookup(z, codebook, table=None, indices=None, out=None, ws=None):
    """hip.vq_lookup: same arguments, same results, CPU tensors; `ws` is not used (one slice or many give the same function)"""
    assert z.dim() == 4 and z.dtype in _TYPES and not z.is_cuda
    assert codebook.dtype == torch.float32 and codebook.dim() == 2 and codebook.shape[1] == z.shape[1]
    assert indices is not None or out is not None
    zr = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    idx = torch.cat([first_strict_min(vq_scores(rows, codebook)) for rows in zr.split(256)])
    P = idx.shape[0]
    if indices is not None:
        assert indices.dtype == torch.int32 and indices.numel() >= P
        indices[:P] = idx.int()
    if out is not None:
        t = codebook if table is None else table
        assert t.dtype == torch.float32 and t.shape[0] == codebook.shape[0] and out.dtype in _TYPES and out.shape[0] >= P and out.shape[1] >= t.shape[1]
        out[:P, :t.shape[1]] = t[idx].to(out.dtype)
        out[:P, t.shape[1]:] = 0


def install(monkeypatch):
    """Replace qdiff.hip.vq_lookup by the emulation (as abi_emulator.install does for the other entry points)."""
    from qdiff import hip
    monkeypatch.setattr(hip, "vq_lookup", vq_lookup)
