"""Torch emulation of qd_mse_search_form / qd_mse_search at the level of qdiff.hip's Python wrapper, for host-logic tests:
include/qdiff_hip.h followed to the letter, one fp32 torch operation per operation of the header's text, in its order.  The
division of the range by `levels` goes through torch's own division by a host scalar — the header's product with the
reciprocal is how ATen evaluates that on the GPU; on the host ATen divides, and so does this.  The terms are fp32, their sum
fp64, divided by the element count and rounded to fp32 once.  The geometry is honoured the way the kernel reads it: through
(rows, cols, ldx) of hip.adaround_rows on the flat storage, so a channel slice is read in place (SEEN records what the entry
saw).  install() patches hip.mse_search and engine.mse_init_device_ok; the entry ticks engine.MSE_INIT_SEARCHES as the
wrapper does.  The product never uses it."""
import torch

SEEN = []            # (rows, cols, ldx, per_row) of every search, as the C entry would receive them
N_CAND = 80


def mse_search_form(rows, cols, per_row):
    if rows <= 0 or cols <= 0:
        return -1
    if not per_row:
        return 2
    return 0 if cols <= 512 else 1


def mse_search(x, per_row, n_bits, n_levels, always_zero, want_scores=False):
    from qdiff import engine, hip
    rows, cols, ldx = hip.adaround_rows(x)
    assert x.dtype == torch.float32 and rows * cols < 2 ** 31
    if not per_row and ldx == cols:
        rows, cols, ldx = 1, rows * cols, rows * cols
    SEEN.append((rows, cols, ldx, bool(per_row)))
    flat = torch.as_strided(x.detach(), (rows, cols), (ldx, 1))        # what the kernel addresses: x + r * ldx + c
    if not per_row:
        flat = flat.reshape(1, -1)
    G, count = flat.shape
    levels, qmax = 2 ** int(n_bits) - 1, int(n_levels) - 1
    factors = hip.mse_factors(x.device)
    x_max, x_min = flat.max(dim=1, keepdim=True)[0], flat.min(dim=1, keepdim=True)[0]
    best = torch.full_like(x_max, 1e+10)
    delta, zero_point = torch.zeros_like(x_max), torch.zeros_like(x_max)
    index = torch.full((G, 1), -1, dtype=torch.int32, device=x.device)
    scores = []
    for i in range(N_CAND):
        hi, lo = x_max * factors[i], x_min * factors[i]
        d = (hi / levels) if always_zero else ((hi - lo) / levels)
        z = torch.zeros_like(d) if always_zero else (-lo / d).round()
        c = torch.clamp(torch.round(flat / d) + z, 0, qmax)
        xq = (c - z) * d
        term = (flat - xq).abs().pow(2.4)
        score = (term.double().sum(dim=1, keepdim=True) / count).float()
        scores.append(score)
        better = score < best
        best = torch.where(better, score, best)
        delta = torch.where(better, d, delta)
        zero_point = torch.where(better, z, zero_point)
        index = torch.where(better, torch.full_like(index, i), index)
    engine.MSE_INIT_SEARCHES[0] += 1
    return (delta.flatten(), zero_point.flatten(), x_min.flatten(), x_max.flatten(), index.flatten(),
            torch.cat(scores, 1) if want_scores else None)


def install(monkeypatch):
    """Route hip.mse_search to the emulation and let host tensors pass engine.mse_init_device_ok; returns the list SEEN."""
    from qdiff import engine, hip
    del SEEN[:]
    monkeypatch.setattr(hip, "mse_search", mse_search)
    monkeypatch.setattr(hip, "mse_search_form", mse_search_form)
    monkeypatch.setattr(engine, "mse_init_device_ok", lambda t: True)
    monkeypatch.setattr(engine, "MSE_INIT_SEARCHES", [0])
    return SEEN
