"""CPU emulation of qd_adaround_fwd / qd_adaround_bwd at the level of qdiff.hip's Python wrappers, for host-logic tests:
include/qdiff_hip.h followed literally, one fp32 torch operation per operation of the header's text, in its order — the
sigmoid s = 1 / (1 + exp(-alpha)) through torch.sigmoid, the composition's own evaluation of it, so that what the host tests
compare with autograd is the Function and the formulas and not two exponentials (the kernel's is judged on the GPU).  The row
geometry is honoured the way the kernel reads it: through (rows, cols, ldw) of hip.adaround_rows on the flat storage, so a
channel slice is read in place.  install() patches the two wrappers and engine.adaround_device_ok; the entry points tick
engine.ADAROUND_LAUNCHES as the wrappers do.  The product never uses it."""
import torch

GW_STRIDES = []          # (cols, ldg) of every adaround_bwd call: tests read whether a gradient slice was taken in place


def _rows(w):
    from qdiff import hip
    rows, cols, ldw = hip.adaround_rows(w)
    flat = torch.as_strided(w, (rows, cols), (ldw, 1))             # what the kernel addresses: w + r * ldw + c
    return flat, rows, cols


def _eval(w, alpha, delta, zp, gamma, zeta):
    flat, rows, cols = _rows(w)
    assert alpha.is_contiguous() and alpha.numel() == rows * cols and delta.shape == zp.shape == (rows,)
    assert flat.dtype == alpha.dtype == delta.dtype == zp.dtype == torch.float32
    d, z, a = delta.view(rows, 1), zp.view(rows, 1), alpha.detach().view(rows, cols)
    zg = float(torch.tensor(float(zeta) - float(gamma), dtype=torch.float32))
    base = torch.floor(flat / d)
    s = torch.sigmoid(a)
    hr = s * zg + gamma
    h = torch.clamp(hr, 0, 1)
    c = (base + h) + z
    return d, z, zg, s, hr, h, c


def adaround_fwd(w, alpha, delta, zero_point, n_levels, gamma, zeta, reg_b=None):
    from qdiff import engine
    d, z, zg, s, hr, h, c = _eval(w, alpha, delta, zero_point, gamma, zeta)
    w_hat = ((torch.clamp(c, 0, n_levels - 1) - z) * d).view(w.shape)
    reg = None
    if reg_b is not None:
        assert reg_b > 0
        reg = (1 - ((h - 0.5).abs() * 2).pow(float(reg_b))).double().sum().float()       # fp32 terms, fp64 sum, one rounding
    engine.ADAROUND_LAUNCHES[0] += 1
    return w_hat, reg


def adaround_bwd(gw, w, alpha, delta, zero_point, n_levels, gamma, zeta, reg_b=None, greg=None):
    from qdiff import engine
    d, z, zg, s, hr, h, c = _eval(w, alpha, delta, zero_point, gamma, zeta)
    from qdiff import hip
    grows, gcols, ldg = hip.adaround_rows(gw)
    assert (grows, gcols) == hr.shape and gw.dtype == torch.float32
    GW_STRIDES.append((gcols, ldg))
    gw = torch.as_strided(gw, (grows, gcols), (ldg, 1))            # read in place, as w
    soft = (hr >= 0) & (hr <= 1)
    zero = torch.zeros((), dtype=torch.float32)
    rec = gw * d
    rec = torch.where((c >= 0) & (c <= n_levels - 1), rec, zero)
    rec = torch.where(soft, rec, zero)
    rec = rec * zg
    rec = (rec * (1 - s)) * s
    if reg_b is not None and greg is not None:
        assert greg.numel() == 1 and greg.dtype == torch.float32
        b = float(reg_b)
        u = h - 0.5
        v = u.abs() * 2
        reg = (-greg.reshape(())) * (b * v.pow(b - 1))
        reg = reg * 2
        reg = reg * torch.sign(u)
        reg = torch.where(soft, reg, zero)
        reg = reg * zg
        reg = (reg * (1 - s)) * s
        rec = rec + reg
    engine.ADAROUND_LAUNCHES[0] += 1
    return rec.view(alpha.shape)


def install(monkeypatch):
    """Route hip.adaround_fwd / adaround_bwd to the emulation and let host tensors pass engine.adaround_device_ok; returns the
    list of entry-point names called."""
    from qdiff import engine, hip
    calls = []

    def fwd(*a, **k):
        calls.append("adaround_fwd")
        return adaround_fwd(*a, **k)

    def bwd(*a, **k):
        calls.append("adaround_bwd")
        return adaround_bwd(*a, **k)

    monkeypatch.setattr(hip, "adaround_fwd", fwd)
    monkeypatch.setattr(hip, "adaround_bwd", bwd)
    monkeypatch.setattr(engine, "adaround_device_ok", lambda t: True)
    monkeypatch.setattr(engine, "ADAROUND_LAUNCHES", [0])
    return calls
