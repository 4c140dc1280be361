"""Cases for the exact tests of the standalone attention matmuls (csrc/bmm_i8.hip: qd_bmm_qk_i8, qd_bmm_pv_i8).  CPU only:
numpy / torch on the host, no device and no import of the library, so the host test can check every condition the GPU test
relies on.

The idea.  Both kernels do exact integer arithmetic, one integer -> fp32 conversion and one fp32 product, so the correct
output is known bit for bit.  A case is built from operand CODES: the stored bytes q8, k8, vt, vsum in the layouts of
qd_quantize_heads (stored byte a' = code - off, "true zero" z' = zp - off; V^T with the key permutation of
abi_emulator._perm_index), the parameter block prm, the fp32 probabilities w and the probability grid.  Expected values come
from the kernels' contract (include/qdiff_hip.h), never from GPU output:

  QK   I[bh,i,j] = sum_{c<d} (q' - zq')(k' - zk')                       int64
       want     = float32(I) * float32(cs)                              numpy's int64 -> float32 (nearest even), one fp32 product
  PV   u        = clamp(rint(float32(w) / float32(dw)) + zpw, wmin, wmax)   evaluated in float32: IEEE division, half-to-even
       I[bh,c,i] = sum_{j<S} (u - zpw)(v' - zv')                        int64
       want     = float32(I) * float32(dw*dv)

The criterion is equality of the bits of every output; nothing is exempt and there is no tolerance.

Pads the contract leaves free are poisoned: random bytes in q rows [T, Tpad), in k rows [S, Spad) (their d-pad columns stay
zero: the constant-operand MFMAs of the zero-point terms sum every column), in V^T rows [d, dpad) and in the V^T slots of the
keys [S, Spad); vsum[d:dpad] = 123456789; NaN in w outside the [T][S] window of every head.  Outputs are allocated by the tests
with a NaN sentinel of a fixed payload; whatever lies outside the written window must still hold it afterwards.

int32 bounds (host test; the kernels' 32-bit intermediates): the QK accumulator holds d*zq'*zk' plus up to three products of
magnitude <= 128 * 128 per padded column; the PV kernel sums a query's codes u - wmin (<= S * (wmax - wmin)) and accumulates the
lo / hi code bytes against v' (<= S * 2^14 each); everything after the accumulators is 64-bit.
"""
import zlib
from types import SimpleNamespace as NS

import numpy as np
import torch

from abi_emulator import _perm_index

SENTINEL_BITS = 0x7FC0DEAD            # a quiet NaN with a payload no arithmetic produces
POISON_SUM = 123456789
INST_D = (4, 32, 40, 64, 68, 96, 100, 128, 132, 160, 228, 256)      # all six DT = dpad / 32, a full and a ragged d-pad each
ZP_SET = (-128, -127, -1, 0, 1, 127)
GEOMETRY = ((1, 1), (31, 77), (32, 32), (33, 31), (129, 97), (160, 33), (1, 97), (129, 1))      # (T, S) at d = 40
GRIDS = ((8, 0, 255), (8, -128, 127), (8, 0, 15), (16, 0, 65535), (16, -32768, 32767))

# the static name list: collection builds nothing, the host test holds it to the builder
CASE_NAMES = (["inst_d%d_p%d" % (d, b) for d in INST_D for b in (8, 16)]
              + ["geom_T%d_S%d" % ts for ts in GEOMETRY]
              + ["zp_d%d_zq%d_zk%d" % (d, zq, zk) for d in (40, 256) for zq in ZP_SET for zk in ZP_SET]
              + ["zv%d_p%d" % (zv, b) for zv in (-128, 0, 127) for b in (8, 16)]
              + ["sat_qk_neg_d256", "sat_qk_pos_d256", "sat_qk_mixed_d256", "sat_pv_p8", "sat_pv_p16"]
              + ["grid_p%d_%d_%d_zpw%d" % (b, lo, hi, z) for b, lo, hi in GRIDS for z in sorted({0, 3, lo, hi})]
              + ["prod_d40_p16", "prod_d256_p8", "prod_d100_p16_split", "prod_d40_p8_scale"])
PRODUCER_NAMES = ("prod_d40_p16", "prod_d256_p8", "prod_d100_p16_split", "prod_d40_p8_scale")


def pad32(n):
    return (n + 31) // 32 * 32


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def is_pow2(x):
    m, _ = np.frexp(np.float32(x))
    return float(m) == 0.5


# ------------------------------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------------------------------
def expect_qk(qs, ks, zq, zk, cs):
    """Stored bytes qs [BH, T, d], ks [BH, S, d] (int64) -> (I int64 [BH, T, S], want float32)."""
    I = np.matmul(qs - zq, np.swapaxes(ks - zk, 1, 2))
    return I, (I.astype(np.float32) * np.float32(cs)).astype(np.float32)


def prob_codes(w, dw, zpw, wmin, wmax):
    """u = clamp(rint(w / dw) + zpw, wmin, wmax) in float32, as int64."""
    with np.errstate(over="ignore"):
        r = np.rint(np.asarray(w, dtype=np.float32) / np.float32(dw)) + np.float32(zpw)
    return np.minimum(np.maximum(r, np.float32(wmin)), np.float32(wmax)).astype(np.int64)


def expect_pv(w, vs, dw, zpw, wmin, wmax, zv, oscale):
    """w float32 [BH, T, S], stored bytes vs [BH, S, d] (int64) -> (u, I int64 [BH, d, T], want float32)."""
    u = prob_codes(w, dw, zpw, wmin, wmax)
    I = np.matmul(np.swapaxes(vs - zv, 1, 2), np.swapaxes(u - zpw, 1, 2))
    return u, I, (I.astype(np.float32) * np.float32(oscale)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# one case from its codes
# ------------------------------------------------------------------------------------------------------------------------
def finish(name, kinds, qs, ks, vs, w, zq=0, zk=0, zv=0, dq=2.0 ** -4, dk=2.0 ** -5, dv=2.0 ** -5, grid=(8, 0, 255), dw=2.0 ** -8,
           zpw=0, lay=None, note="", floats=None, scale=1.0):
    """qs [BH, T, d], ks / vs [BH, S, d]: stored bytes (int64 in [-128, 127]); w float32 [BH, T, S]; z*: stored zero points.
    lay: row / head paddings of the strided operands (elements): qk_ldo, qk_rows, pv_ldo, pv_rows, ldw, w_rows."""
    rng = _rng(name + "/pads")
    BH, T, d = qs.shape
    S = ks.shape[1]
    Tpad, Spad, dpad = pad32(T), pad32(S), pad32(d)
    wbits, wmin, wmax = grid
    for a in (qs, ks, vs):
        assert a.dtype == np.int64 and a.min() >= -128 and a.max() <= 127, name
    assert all(-128 <= z <= 127 for z in (zq, zk, zv)) and wmin <= zpw <= wmax and wmax - wmin <= 2 ** wbits - 1, name
    rnd = lambda *shape: rng.integers(-128, 128, size=shape)
    q8 = np.zeros((BH, Tpad, dpad), dtype=np.int64)
    q8[:, :T, :d] = qs
    q8[:, T:, :] = rnd(BH, Tpad - T, dpad)
    k8 = np.zeros((BH, Spad, dpad), dtype=np.int64)
    k8[:, :S, :d] = ks
    k8[:, S:, :d] = rnd(BH, Spad - S, d)
    nat = np.zeros((BH, dpad, Spad), dtype=np.int64)                     # V^T in natural key order
    nat[:, :d, :S] = np.swapaxes(vs, 1, 2)
    nat[:, d:, :] = rnd(BH, dpad - d, Spad)
    nat[:, :, S:] = rnd(BH, dpad, Spad - S)
    vt = nat[:, :, _perm_index(Spad).numpy()]                            # slot p holds key _perm_index[p]
    vsum = np.full((BH, dpad), POISON_SUM, dtype=np.int64)
    vsum[:, :d] = vs.sum(1)
    cs = np.float32(np.float32(dq) * np.float32(dk))                     # as the engine forms prm[0] and prm[5]: fp32 products
    oscale = np.float32(np.float32(dw) * np.float32(dv))
    prm = np.zeros(8, dtype=np.float32)
    prm[:7] = [cs, zq, zk, np.float32(dw), zpw, oscale, zv]
    L = dict(qk_ldo=S, qk_rows=T, pv_ldo=T, pv_rows=d, ldw=S, w_rows=T)
    L.update(lay or {})
    w = np.asarray(w, dtype=np.float32)
    assert w.shape == (BH, T, S) and np.isfinite(w).all(), name
    w_full = np.full((BH, L["w_rows"], L["ldw"]), np.nan, dtype=np.float32)
    w_full[:, :T, :S] = w
    I_qk, want_qk = expect_qk(qs, ks, zq, zk, cs)
    u, I_pv, want_pv = expect_pv(w, vs, dw, zpw, wmin, wmax, zv, oscale)
    t8 = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int8)))      # the kernels address raw memory: row-major, always
    return NS(name=name, kinds=tuple(kinds), BH=BH, T=T, S=S, d=d, Tpad=Tpad, Spad=Spad, dpad=dpad, DT=dpad // 32,
              q8=t8(q8), k8=t8(k8), vt=t8(vt), vsum=torch.from_numpy(vsum.astype(np.int32)), prm=torch.from_numpy(prm),
              w_full=torch.from_numpy(w_full), grid=tuple(grid), wbits=wbits, wmin=wmin, wmax=wmax, lay=NS(**L),
              qs=qs, ks=ks, vs=vs, u=u, zq=zq, zk=zk, zv=zv, zpw=zpw, dq=float(np.float32(dq)), dk=float(np.float32(dk)),
              dv=float(np.float32(dv)), dw=float(np.float32(dw)), cs=float(cs), oscale=float(oscale),
              I_qk=I_qk, want_qk=torch.from_numpy(want_qk), I_pv=I_pv, want_pv=torch.from_numpy(want_pv),
              w_sym=wmin < 0, w_nbits=int(wmax - wmin).bit_length(), note=note, floats=floats, scale=float(scale))


def w_view(c, w_full=None):
    """The [BH][T][S] window of the probabilities (strides carry ldw and the head stride)."""
    return (c.w_full if w_full is None else w_full)[:, :c.T, :c.S]


def int32_bounds(c):
    """Upper bounds of the kernels' 32-bit intermediates for this case (module docstring)."""
    b = {}
    if "qk" in c.kinds:
        b["qk_accumulator"] = c.d * abs(c.zq * c.zk) + c.dpad * 128 * (128 + abs(c.zq) + abs(c.zk))
        b["qk_I"] = int(np.abs(c.I_qk).max())
    if "pv" in c.kinds:
        b["pv_code_sum"] = int((c.u - c.wmin).sum(-1).max())
        b["pv_code_sum_bound"] = c.S * (c.wmax - c.wmin)
        b["pv_byte_accumulators"] = c.S * 2 ** 14
        b["pv_I"] = int(np.abs(c.I_pv).max())
    return b


# ------------------------------------------------------------------------------------------------------------------------
# content
# ------------------------------------------------------------------------------------------------------------------------
NP2 = dict(dq=0.0371, dk=0.0519, dv=0.0437)                  # step sizes that are no powers of two: cs and dw*dv round


def _bytes(rng, *shape):
    return rng.integers(-128, 128, size=shape)


def _probs(rng, BH, T, S):
    """Probabilities over the whole grid: mostly small, some near 1, exact 0 and 1, one value above the grid."""
    w = (rng.random((BH, T, S)) ** 3).astype(np.float32)
    w[rng.random((BH, T, S)) < 0.05] = 0.0
    w[rng.random((BH, T, S)) < 0.03] = 1.0
    w[:, T // 2, S // 2] = 1.5
    return w


def _dw(wbits, wmin, wmax, pow2):
    return 2.0 ** -(wmax - wmin).bit_length() if pow2 else float(np.float32(1.0 / (wmax - wmin)))


def case_random(name, BH, T, S, d, wbits, zq, zk, zv, kinds=("qk", "pv"), pow2=False, lay=None, note=""):
    rng = _rng(name)
    grid = (wbits, 0, 2 ** wbits - 1)
    steps = dict(dq=2.0 ** -4, dk=2.0 ** -6, dv=2.0 ** -5) if pow2 else NP2
    return finish(name, kinds, _bytes(rng, BH, T, d), _bytes(rng, BH, S, d), _bytes(rng, BH, S, d), _probs(rng, BH, T, S), zq, zk, zv,
                  grid=grid, dw=_dw(*grid, pow2), lay=lay, note=note, **steps)


def case_instantiation(d, wbits):
    """bmm_qk_kernel<DT> and bmm_pv_kernel<DT, wbits == 16> on random codes, asymmetric zero points, non power-of-two scales."""
    return case_random("inst_d%d_p%d" % (d, wbits), 3, 33, 33, d, wbits, zq=-11 - d % 7, zk=23 + d % 5, zv=-37 + d % 11,
                       note="every instantiation")


def case_geometry(T, S):
    name = "geom_T%d_S%d" % (T, S)
    n = GEOMETRY.index((T, S))
    BH, lay, note = 3, None, "row / key counts around the 32-wide tile and the 128-query block"
    if (T, S) == (1, 1):
        BH, note = 1, "one head, one query, one key"
    if (T, S) == (129, 97):
        BH, lay = 5, dict(qk_ldo=S + 7, qk_rows=T + 2, pv_ldo=T + 3, pv_rows=40 + 5)
        note = "five heads; output rows and heads padded (ldo > S / T, head stride > rows * ldo)"
    if (T, S) == (31, 77):
        lay, note = dict(ldw=S + 5, w_rows=T + 3), "probabilities with ldw > S and a larger head stride"
    return case_random(name, BH, T, S, 40, (8, 16)[n % 2], zq=5, zk=-9, zv=17, pow2=(n % 4 == 3), lay=lay, note=note)


def case_zero_points(d, zq, zk):
    """The d*zq'*zk' seed and the constant-operand MFMAs: -z' = 128 takes two byte constants, z' = 0 skips the branch."""
    return case_random("zp_d%d_zq%d_zk%d" % (d, zq, zk), 3, 33, 33, d, 8, zq, zk, 0, kinds=("qk",), pow2=(d == 256 and zq < 0),
                       note="zero-point paths of the QK kernel")


def case_zv(zv, wbits):
    return case_random("zv%d_p%d" % (zv, wbits), 3, 33, 33, 40, wbits, 0, 0, zv, kinds=("pv",), note="v zero point at the grid ends")


def case_saturated_qk(which):
    BH, T, S, d = 3, 33, 33, 256
    rng = _rng("sat_qk_" + which)
    if which == "neg":
        qs, ks, zq, zk = np.full((BH, T, d), -128), np.full((BH, S, d), -128), 127, 127
    elif which == "pos":
        qs, ks, zq, zk = np.full((BH, T, d), 127), np.full((BH, S, d), 127), -128, -128
    else:                                                              # head 0: q~ = -255 against k~ = +255; others: random end codes
        ends = lambda *shape: np.where(rng.integers(0, 2, size=shape) == 1, 127, -128)
        qs, ks, zq, zk = ends(BH, T, d), ends(BH, S, d), 127, -128
        qs[0], ks[0] = -128, 127
    return finish("sat_qk_%s_d256" % which, ("qk",), qs.astype(np.int64), ks.astype(np.int64), _bytes(rng, BH, S, d), _probs(rng, BH, T, S),
                  zq, zk, 0, note="end codes against the far zero point: |I| = 256 * 255 * 255", **NP2)


def case_saturated_pv(wbits):
    """Every probability above the clamp (code wmax) against v' = -128, zv' = 127 over S = 97 keys."""
    BH, T, S, d = 3, 33, 97, 40
    rng = _rng("sat_pv_%d" % wbits)
    grid = (wbits, 0, 2 ** wbits - 1)
    return finish("sat_pv_p%d" % wbits, ("pv",), _bytes(rng, BH, T, d), _bytes(rng, BH, S, d), np.full((BH, S, d), -128, dtype=np.int64),
                  np.full((BH, T, S), 2.0, dtype=np.float32), 0, 0, 127, grid=grid, dw=2.0 ** -wbits,
                  note="all codes at wmax, |v~| = 255", **NP2)


GRID_ROWS = dict(zero_one=0, ties_even=1, ties_odd=2, above=3, to_wmin=4, softmax=5)


def grid_probs(rng, BH, T, S, dw, zpw, wmin, wmax):
    """Probabilities for one grid; feature rows (GRID_ROWS) sit at row (r + 7 * bh) % T of head bh.  lo / hi: the range of
    rint(w / dw) that the clamp leaves alone."""
    lo, hi = wmin - zpw, wmax - zpw
    w = (rng.uniform(lo - 2, hi + 2, size=(BH, T, S)) * dw).astype(np.float32)
    for bh in range(BH):
        row = lambda key: (GRID_ROWS[key] + 7 * bh) % T
        w[bh, row("zero_one")] = np.arange(S) % 2
        n = np.arange(lo, hi)                                          # n + 0.5 rounds to n or n + 1, both on the grid
        for key, parity in (("ties_even", 0), ("ties_odd", 1)):
            pool = n[n % 2 == parity]
            pick = rng.choice(pool, size=S)
            pick[0], pick[1] = pool[0], pool[-1]
            w[bh, row(key)] = (pick + 0.5) * dw
        w[bh, row("above")] = (hi + 0.6 + 100 * rng.random(S)) * dw
        w[bh, row("above"), ::5] = 1.0e6
        below = np.array([lo - 0.4, lo + 0.3, lo - 1000.0, lo + 0.49, lo - 0.5])
        w[bh, row("to_wmin")] = below[np.arange(S) % 5] * dw
        w[bh, row("to_wmin"), 3] = -1.0e6
        e = np.exp(3.0 * rng.standard_normal(S))
        w[bh, row("softmax")] = (e / e.sum()).astype(np.float32)
    return w


def case_grid(wbits, wmin, wmax, zpw):
    name = "grid_p%d_%d_%d_zpw%d" % (wbits, wmin, wmax, zpw)
    rng = _rng(name)
    BH, T, S, d = 3, 33, 40, 40
    dw = _dw(wbits, wmin, wmax, True)                                  # a power of two: (n + 0.5) * dw is an exact tie
    return finish(name, ("pv",), _bytes(rng, BH, T, d), _bytes(rng, BH, S, d), _bytes(rng, BH, S, d),
                  grid_probs(rng, BH, T, S, dw, zpw, wmin, wmax), 0, 0, -23, grid=(wbits, wmin, wmax), dw=dw, zpw=zpw,
                  note="probability grid, zero point and rounding edges of the P.V epilogue", **NP2)


def case_producer(name, d, wbits, T, S, zq, zk, zv):
    """Codes that float inputs x = (code - zp) * delta reproduce exactly in the quantiser: power-of-two step sizes."""
    return case_random(name, 3, T, S, d, wbits, zq, zk, zv, pow2=True, note="also run through qd_quantize_heads from float inputs")


def case_producer_scale():
    """Step sizes that are no powers of two and a `scale`: the codes are those of (x * scale) / delta evaluated in float32."""
    name = "prod_d40_p8_scale"
    rng = _rng(name)
    BH, T, S, d = 3, 33, 45, 40
    scale = float(np.float32(40 ** -0.25))
    zq, zk, zv = 9, -21, 30
    grid = (8, 0, 255)
    xs = {}
    stored = {}
    for key, L, delta, z, pre in (("q", T, NP2["dq"], zq, scale), ("k", S, NP2["dk"], zk, scale), ("v", S, NP2["dv"], zv, 1.0)):
        x = (rng.standard_normal((BH, d, L)) * 110 * delta / pre).astype(np.float32)           # "bct"; some codes clamp
        y = (x * np.float32(pre)).astype(np.float32) / np.float32(delta)
        code = np.clip(np.rint(y) + np.float32(z + 128), 0, 255).astype(np.int64)
        xs[key], stored[key] = x, np.ascontiguousarray(np.swapaxes(code - 128, 1, 2))
    return finish(name, ("qk", "pv"), stored["q"], stored["k"], stored["v"], _probs(rng, BH, T, S), zq, zk, zv, grid=grid,
                  dw=_dw(*grid, False), floats=xs, scale=scale, note="float inputs, non power-of-two step sizes and a scale", **NP2)


def build_cases():
    cases = [lambda d=d, b=b: case_instantiation(d, b) for d in INST_D for b in (8, 16)]
    cases += [lambda T=T, S=S: case_geometry(T, S) for T, S in GEOMETRY]
    cases += [lambda d=d, zq=zq, zk=zk: case_zero_points(d, zq, zk) for d in (40, 256) for zq in ZP_SET for zk in ZP_SET]
    cases += [lambda zv=zv, b=b: case_zv(zv, b) for zv in (-128, 0, 127) for b in (8, 16)]
    cases += [lambda w=w: case_saturated_qk(w) for w in ("neg", "pos", "mixed")]
    cases += [lambda b=b: case_saturated_pv(b) for b in (8, 16)]
    cases += [lambda g=g, z=z: case_grid(*g, z) for g in GRIDS for z in sorted({0, 3, g[1], g[2]})]
    cases += [lambda: case_producer("prod_d40_p16", 40, 16, 33, 45, 5, -9, 17),
              lambda: case_producer("prod_d256_p8", 256, 8, 33, 45, -128, 127, -128),
              lambda: case_producer("prod_d100_p16_split", 100, 16, 45, 45, 31, -2, 64),
              case_producer_scale]
    return cases


_CACHE = {}


def all_cases():
    """Every case, built once per process (a dict name -> case, in definition order)."""
    if "cases" not in _CACHE:
        out = {}
        for fn in build_cases():
            c = fn()
            assert c.name not in out, c.name
            out[c.name] = c
        _CACHE["cases"] = out
    return _CACHE["cases"]


# ------------------------------------------------------------------------------------------------------------------------
# outputs: sentinel buffers and the criterion
# ------------------------------------------------------------------------------------------------------------------------
def sentinel(shape, device="cpu"):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device=device).view(torch.float32)


def out_buffers(c, kind, device="cpu"):
    """(whole buffer filled with the sentinel, the [BH][rows][cols] window the kernel writes)."""
    if kind == "qk":
        full = sentinel((c.BH, c.lay.qk_rows, c.lay.qk_ldo), device)
        return full, full[:, :c.T, :c.S]
    full = sentinel((c.BH, c.lay.pv_rows, c.lay.pv_ldo), device)
    return full, full[:, :c.d, :c.T]


def check_output(c, kind, full):
    """Bit equality inside the window, the sentinel everywhere else.  Returns (ok, report)."""
    full = full.cpu()
    want = c.want_qk if kind == "qk" else c.want_pv
    R, C = want.shape[1:]
    bits = full.view(torch.int32)
    inside = torch.zeros(full.shape, dtype=torch.bool)
    inside[:, :R, :C] = True
    got = bits[:, :R, :C]
    bad = got != want.view(torch.int32)
    spilled = (bits != SENTINEL_BITS) & ~inside
    first = None
    if bad.any():
        i = tuple(int(x) for x in bad.nonzero()[0])
        I = c.I_qk if kind == "qk" else c.I_pv
        first = dict(element=i, I=int(I[i]), got=float(full[i]), want=float(want[i]))
    rep = NS(compared=int(bad.numel()), mismatches=int(bad.sum()), spilled=int(spilled.sum()), first=first)
    return rep.mismatches == 0 and rep.spilled == 0, rep
