"""Helpers of tests/test_value_edges_gpu.py: edge-value vectors for a quantiser grid and the tie-aware code comparison.

Tie-aware comparison.  The fp64 quotient u = y / delta + zp of the exact (fp64) pre-quantiser value y decides the oracle's
code clamp(round_half_even(u), qmin, qmax).  A kernel that computes y in fp32 may land on the other side of a rounding
boundary — a half-integer inside the grid, or qmin - 0.5 / qmax + 0.5 — only when u lies within `w` of that boundary, where w is
the kernel's own error bound on y divided by delta (derived per test; a scalar, or a tensor of u's shape where the bound
depends on the element).  Its code may then differ from the oracle's by exactly one, and only towards that boundary (the side
u would cross); everywhere else the codes must be equal.  A pure quantiser has w = 0 and is compared bit for bit instead.
"""
import itertools
import struct

import pytest
import torch


def f32_from_bits(b):
    return struct.unpack("f", struct.pack("I", b))[0]


def nearest_boundary(u, qmin, qmax):
    """The rounding boundary of the grid [qmin, qmax] nearest to every fp64 quotient u: the half-integer floor(u) + 0.5, or
    qmin - 0.5 / qmax + 0.5 beyond the grid."""
    return (torch.floor(u) + 0.5).clamp(qmin - 0.5, qmax + 0.5)


def oracle_codes(u, qmin, qmax):
    return torch.round(u).clamp(qmin, qmax).long()


def tie_aware_check(name, got, u, qmin, qmax, w, record=None):
    """got: integer codes (int64, zero point included); u: fp64 quotients of the same shape; w: the window, a float or a
    tensor of u's shape.  Asserts the rule of the module docstring and returns (accepted mismatches, largest accepted
    distance).  record: pytest's record_property — the counts land in the test report (junit XML) as well as on stdout."""
    got = got.long().reshape(-1)
    u = u.double().reshape(-1)
    wt = w.double().reshape(-1) if torch.is_tensor(w) else torch.full_like(u, float(w))
    w = float(wt.max()) if wt.numel() else 0.0
    want = oracle_codes(u, qmin, qmax)
    b = nearest_boundary(u, qmin, qmax)
    dist = (u - b).abs()
    # a code off by one is accepted only on the far side of the nearest boundary, within w of it
    toward = torch.sign(b - u).long()
    ok1 = ((got - want) == toward) & (toward != 0) & (dist <= wt)
    bad = (got != want) & ~ok1
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} codes differ outside the tie window "
                             f"(first at {i}: got {int(got[i])}, want {int(want[i])}, u={float(u[i]):.9g}, distance {float(dist[i]):.3g}, "
                             f"w there {float(wt[i]):.3g})")
    n, mx = int(ok1.sum()), (float(dist[ok1].max()) if bool(ok1.any()) else 0.0)
    if record is not None:
        record(f"tie_window[{name}]", f"{n} of {got.numel()} accepted, largest distance {mx:.3g}, w {w:.3g}")
    print(f"\n[tie-window] {name}: {n} of {got.numel()} codes accepted off by one, largest distance {mx:.3g} (w <= {w:.3g})")
    return n, mx


def edge_values(delta, zp, qmin, qmax, n_random, g, half=False):
    """fp32 values at the edges of the grid (delta, zp, [qmin, qmax]):
    exact ties (k + 0.5) * delta whose fp32 division is exactly the tie (checked here), the clamp boundaries
    (qmin - zp +- 0.5) * delta and (qmax - zp +- 0.5) * delta with their fp32 neighbours, +-0, huge finite values, +-inf,
    plus n_random values spread over 1.6x the grid (so a share of them clip).  Returns (values, number of exact ties)."""
    dt = torch.tensor(delta, dtype=torch.float32)
    d = float(dt)
    ks = torch.arange(qmin - zp - 2, qmax - zp + 2, dtype=torch.float64)
    cand = ((ks + 0.5) * d).float()
    if half:
        cand = cand.half().float()
    ties = cand[(cand / dt).double() == ks + 0.5]
    edges = []
    for k in (qmin - zp - 0.5, qmin - zp + 0.5, qmax - zp - 0.5, qmax - zp + 0.5, qmin - zp, qmax - zp):
        v = torch.tensor(k * d, dtype=torch.float32)
        edges += [float(v), float(torch.nextafter(v, torch.tensor(float("inf")))), float(torch.nextafter(v, torch.tensor(float("-inf"))))]
    big = [0.0, -0.0, 1e-30, -1e-30, 1e4, -1e4, 6.5e4, -6.5e4, 1e30, -1e30, 3e38, -3e38, 3.4028235e38, -3.4028235e38,
           float("inf"), float("-inf")]
    span = (qmax - qmin + 1) * d
    rnd = (torch.rand(n_random, generator=g, dtype=torch.float64) * 1.6 - 0.3) * span + (qmin - zp) * d
    v = torch.cat([ties, torch.tensor(edges + big, dtype=torch.float32), rnd.float()])
    if half:
        v = v.half().float()
    return v, int(ties.numel())


def params(*axes):
    """pytest parameters over the product of `axes`, each a list of (id, value): the test id joins the ids in axis order, and
    an id of None is left out — an axis added to an existing test lists its original value first with id None, so every case
    the test had before keeps its id."""
    out = []
    for combo in itertools.product(*axes):
        out.append(pytest.param(*[v for _, v in combo], id="-".join(i for i, _ in combo if i is not None)))
    return out


def device_rows(x, ldx, shift, dtype, device):
    """x: [M][C] fp32 (already representable in dtype) -> rows of `dtype` on `device` with leading dimension ldx whose first
    element lies `shift` elements past the start of a fresh (256-byte aligned) allocation."""
    M, C = x.shape
    buf = torch.zeros(shift + M * ldx, dtype=dtype, device=device)
    rows = buf[shift:].view(M, ldx)[:, :C]
    rows.copy_(x.to(device=device, dtype=dtype))
    return rows
