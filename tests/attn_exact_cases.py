"""Cases for the exact-row tests of the fused int8 attention (csrc/attn_i8.hip).  CPU only: numpy / torch on the host, no
device and no import of the library, so the host test can check every condition the GPU test relies on.

The idea.  The kernel's only floating-point work is the softmax; every other step is exact integer arithmetic.  A case
therefore starts from operand CODES (float inputs x = (code - zp) * delta with power-of-two deltas reproduce them exactly in
the quantiser), computes exact int64 scores, an fp64 softmax, and c_j = p_j / dw + ubias (ubias = zpw - wmin: the kernel
rounds uu = c_j to an integer in [0, wmax - wmin], the probability code is uu + wmin).  A key is DECIDED when c_j is further
than the margin m_j from every half-integer, or lies above the clamp's last tie (c_j > urange - 0.5 + m_j); a row is decided
when all its S keys are.  On a decided row the integer I = sum_j (u_j - zpw)(v_j - zv) is known and the kernel must return
float32(I) * float32(dw*dv) (one correctly rounded int -> fp32 conversion, one fp32 product; bit-exact when dw and dv are
powers of two).  On other rows every undecided code may be either neighbour: |got - want| <= dw*dv * sum_undecided |v_j - zv|.

The margin m_j (derived from the kernel's expressions, never fitted to GPU output).  u = 2^-24 is half an fp32 ulp (one
rounding); E = 2u bounds v_exp_f32, whose accuracy neither the ISA text nor the microarchitecture guide at hand states:
1 ulp is ASSUMED.  cs = prm[0] is exact in every case (power-of-two deltas, an fp32-representable `scale`; asserted).
L_j = cs*log2(e)*(max - s_j) >= 0 is the distance of key j below the row maximum in octaves.

  scores -> log2 domain.  cs2 = fl(prm[0] * fl(log2 e)) carries two roundings, a SYSTEMATIC relative error 2u: an error
      2u*L in any exponent that spans L octaves.  attn_kernel: x = fl(float(s - max) * cs2), one more rounding, u*L_j.  Lean /
      LDS bodies: x = fma(F, cs2, nc) = fl(cs2*(s - m) + eps(m)) with |eps| <= cs2, again one rounding, u*(L_j + cs2); 2^eps
      cancels against the normaliser (attn_finish_stats) up to the roundings counted below.
      => exponent error of key j in sweep 2:  u * (3*L_j + cs2),  relative error of e_j:  ln2 * that + E.
  normaliser.  All terms are positive, so the relative error of the sum is a p-weighted mean of the terms' errors plus what
      the additions add:
      * each term's own exponent error, as above but against the reference of sweep 1 (attn_kernel: the running maximum;
        lean: m0, the maximum of tile 0), which lies up to `rise` octaves below the row maximum:
        ln2 * 3u * (Lw + rise), Lw = sum_j p_j L_j;  rise = cs2 * (row max - maximum of tile 0) for the lean bodies; attn_kernel
        keeps one running maximum per half-wave: sum_h P_h * cs2 * (the half's maximum - its tile-0 maximum), P_h the half's
        share of the row (how far the half lies below the row maximum is the cross-half item below); the larger of the two;
      * attn_kernel's rescales: shift = fl(up * cs2) is used by the new terms and by exp2(-shift) alike, so its rounding is a
        factor common to everything summed so far: u * cs2 * sum(up) <= u * rise in the exponent.  Lean: fl(mx * cs2) and
        the subtraction from (eps - eps0): 2u * (rise + 2*cs2);
      * the cross-half combination of attn_kernel: half h contributes P_h <= min(1, 16*ntile * 2^-g) at exponent error 3u*g
        (g: its maximum's distance below the row's): P_h * g <= log2(S) + 2;
      => ln2 * u * (3*Lw + 5*rise + log2(S) + 2 + 4*cs2);
      * every multiplication, exp2 and addition on a term's way into l:  attn_kernel rescales l once per tile (one product
        rounding + E of exp2(-shift)): ntile * (u + E); the rest (own exp2, a2.x + a2.y, l*f + a, the cross-half exp2,
        product and add; lean: own exp2, a2.x + a2.y, l + lo, exp2, product) is bounded by 14u + 3E for both families;
      * the additions themselves: fl(a + t) errs by at most min(u*(a + t), t) (a is representable).  A row's keys are summed
        in four independent chains (half-wave x the two lanes of the packed add: chain(j) = (bit 2 of j, bit 0 of j)), the
        partial sum of a chain never exceeds the chain's share w_c of l, so the key-level adds cost
        sum_j min(u * w_chain(j), p_j) relative to l; the adds of per-tile partial sums (attn_kernel) cost at most
        min(ntile * u, sigma), sigma = sum_j min(u, p_j) (min is subadditive), the last three adds 3u (counted above).  A row
        with a handful of live keys pays for those only; terms that v_exp_f32 flushes to zero (x < -126) are inside sigma.
      => rel_norm = ln2*u*(3*Lw + 5*rise + log2 S + 2 + 4*cs2) + ntile*(u + E) + 14u + 3E + adds.
  inv = 1 / fl(l * dw): one product rounding and a correctly rounded division (the library is built with
      -fhip-fp32-correctly-rounded-divide-sqrt): 2u.
  t = fma(e, inv, ubias): exact product inside; in the clamped body the sum is rounded to fp32 BEFORE the + MAGIC rounding
      to an integer (double rounding): u * (c_j + ubias).  The unclamped bodies round once; the margin covers both, so the
      wave-uniform choice of body (which pad query rows may sway) does not matter on decided keys.
      + MAGIC is the round-half-even under test; exact ties are never decided.
  => m_j = 1.01 * [ c_j * (rel_norm + ln2*u*(3*L_j + cs2) + E + 2u) + u * (c_j + ubias + 1) ] + 2^-60.
  (1.01: second-order terms; 2^-60: absolute slack for flushed subnormals, e_j * inv < 2^-126 * 2^32.)  m_j is positive and
  grows with the code.

Constructions.  "designed" rows: a few leading head dims carry one-hot (or hi/lo grid) key signatures at magnitude 127, so
that query i gives chosen keys chosen integer scores and every other key lies tens of octaves below (code 0 by far more than
m_j); the remaining dims hold random codes on one side and the zero point on the other (they contribute exactly nothing to
q~.k~ but fill the operand bytes the MFMAs and the zero-point restoration read).  "dense" rows: random small q~, k~ on all
dims; rows that are not decided get their query codes redrawn (fixed seed, at most REDRAWS rounds).
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

U = 2.0 ** -24
EXP = 2.0 * U                  # v_exp_f32: 1 ulp assumed
LOG2E = math.log2(math.e)
LN2 = math.log(2.0)
REDRAWS = 24


def _grid(n_bits, sym):
    nl = 2 ** (n_bits - 1) - 1
    return (-nl - 1, nl) if sym else (0, 2 ** n_bits - 1)


def margin(c, L, Lw, rise, adds, S, cs2, ubias):
    """m_j of the module docstring; c, L: [.., S]; Lw, rise, adds: [.., 1]."""
    ntile = (S + 31) // 32
    rel_norm = LN2 * U * (3 * Lw + 5 * rise + math.log2(S) + 2 + 4 * cs2) + ntile * (U + EXP) + 14 * U + 3 * EXP + adds
    rel_key = LN2 * U * (3 * L + cs2) + EXP + 2 * U
    return 1.01 * (c * (rel_norm + rel_key) + U * (c + ubias + 1)) + 2.0 ** -60


def softmax_codes(s, cs, dw, zpw, wmin, wmax):
    """s: exact int64 scores [N, T, S] -> (uu - ubias int64, decided keys bool, margin, c) with an fp64 softmax."""
    S = s.shape[-1]
    cs2 = cs * LOG2E
    ubias = float(zpw - wmin)
    urange = float(wmax - wmin)
    smax = s.max(-1, keepdims=True)
    L = (smax - s).astype(np.float64) * cs2
    e = np.exp2(-L)
    p = e / e.sum(-1, keepdims=True)
    c = p / dw
    Lw = (p * L).sum(-1, keepdims=True)
    sigma = np.minimum(p, U).sum(-1, keepdims=True)
    jj = np.arange(S)
    chain = ((jj >> 2) & 1) * 2 + (jj & 1)
    adds = np.minimum(((S + 31) // 32) * U, sigma)
    for ch in range(4):
        sel = chain == ch
        if sel.any():
            adds = adds + np.minimum(U * p[..., sel].sum(-1, keepdims=True), p[..., sel]).sum(-1, keepdims=True)
    # rise: lean / LDS bodies sum against m0 = the maximum of tile 0 (both half-waves); attn_kernel keeps a running maximum per
    # half-wave (keys e + 8g + 4*half of a 32-key tile), whose rescale errors weigh with the half's share P_h of the row
    jj0 = jj[:min(32, S)]
    rise = (smax - s[..., jj0].max(-1, keepdims=True)).astype(np.float64) * cs2
    rise_a = np.zeros_like(rise)
    for half in (0, 1):
        sel = ((jj >> 2) & 1) == half
        sel0 = sel[:min(32, S)]
        if sel0.any():
            own = s[..., sel].max(-1, keepdims=True) - s[..., jj0[sel0]].max(-1, keepdims=True)
            rise_a = rise_a + p[..., sel].sum(-1, keepdims=True) * own.astype(np.float64) * cs2
    rise = np.maximum(rise, rise_a)
    m = margin(c, L, Lw, rise, adds, S, cs2, ubias)
    t = c + ubias
    tie = np.abs(t - np.floor(t) - 0.5)
    decided = (tie > m) | (t > urange - 0.5 + m)
    uu = np.minimum(np.rint(t), urange)
    return (uu - ubias).astype(np.int64), decided, m, c


def _exact_matmul(a, b):
    """Integer-valued contraction in fp64 BLAS: exact while |sums| < 2^53 (asserted)."""
    r = np.matmul(a.astype(np.float64), b.astype(np.float64))
    assert np.abs(r).max() < 2.0 ** 52
    return np.rint(r).astype(np.int64)


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def evaluate(spec, qc, kc, vc):
    """Everything the tests need from the codes: exact I, decided rows, tolerances."""
    zq, zk, zv = spec.zq, spec.zk, spec.zv
    s = _exact_matmul(qc - zq, np.swapaxes(kc - zk, 1, 2))
    pu, dec_keys, m, c = softmax_codes(s, spec.cs, spec.dw, spec.zpw, spec.wmin, spec.wmax)
    I = _exact_matmul(pu, vc - zv)
    und = ~dec_keys
    tol = spec.dw * spec.dv * np.matmul(und.astype(np.float64), np.abs(vc - zv).astype(np.float64))
    return NS(s=s, pu=pu, dec_keys=dec_keys, m=m, c=c, I=I, decided=dec_keys.all(-1), tol=tol, undecided_per_row=und.sum(-1))


def _to_float(codes, zp, delta, B, H, prescale=1.0):
    """[B*H, L, d] codes -> float32 [B, L, H*d] with x * prescale = (code - zp) * delta exactly."""
    BH, L, d = codes.shape
    x = (codes - zp).astype(np.float64) * (delta / prescale)
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    return torch.from_numpy(np.ascontiguousarray(x32.reshape(B, H, L, d).transpose(0, 2, 1, 3).reshape(B, L, H * d)))


class Spec:
    """Shape, grids and quantiser parameters of one case."""

    def __init__(self, name, B, H, T, S, d, wbits=16, wsym=False, zpw=0, dw=2.0 ** -16, qsym=False, zq=117, zk=140, zv=97,
                 cs=2.0 ** -9, scale=1.0, prescale=1.0, dv=2.0 ** -5, seed=0, forms=None):
        self.name, self.B, self.H, self.T, self.S, self.d = name, B, H, T, S, d
        self.BH = B * H
        self.wbits, self.wsym, self.zpw, self.dw = wbits, wsym, zpw, float(dw)
        self.wmin, self.wmax = _grid(wbits, wsym)
        self.qsym = qsym
        self.qmin, self.qmax = _grid(8, qsym)
        self.zq, self.zk, self.zv = (0, 0, 0) if qsym else (zq, zk, zv)
        self.cs, self.scale, self.prescale, self.dv = float(cs), float(scale), float(prescale), float(dv)
        # cs = dq * dk * scale with dq = 2^-4 fixed: dk absorbs the rest and must stay a power of two
        self.dq = 2.0 ** -4
        self.dk = self.cs / (self.dq * self.scale)
        self.seed = seed
        self.forms = forms
        self.rng = np.random.default_rng(1000 + seed)

    def tilde_range(self, zp):
        return self.qmin - zp, self.qmax - zp


def finish(spec, qc, kc, vc, features, note="", stated_undecided=False):
    for codes in (qc, kc, vc):
        assert codes.min() >= spec.qmin and codes.max() <= spec.qmax
    ev = evaluate(spec, qc, kc, vc)
    f32 = lambda x: float(np.float32(x))
    # prm[0] and prm[5] as the plan builder forms them (fp32 products): cs must be exact, dw*dv is what the kernel multiplies by
    cs32 = f32(np.float32(np.float32(spec.dq) * np.float32(spec.dk)) * np.float32(spec.scale))
    assert cs32 == spec.cs and f32(spec.scale) == spec.scale and f32(spec.dw) == spec.dw, spec.name
    oscale = np.float32(np.float32(spec.dw) * np.float32(spec.dv))
    want = (ev.I.astype(np.float32) * oscale).astype(np.float32)                 # int64 -> fp32 is round-to-nearest-even
    pow2 = math.frexp(spec.dw)[0] == 0.5 and math.frexp(spec.dv)[0] == 0.5
    mk = lambda delta, zp, bits, sym: dict(delta=torch.tensor(delta, dtype=torch.float32), zero_point=int(zp), n_bits=bits, sym=sym)
    case = NS(name=spec.name, B=spec.B, H=spec.H, T=spec.T, S=spec.S, d=spec.d, spec=spec,
              q=_to_float(qc, spec.zq, spec.dq, spec.B, spec.H, spec.prescale),
              k=_to_float(kc, spec.zk, spec.dk, spec.B, spec.H, spec.prescale),
              v=_to_float(vc, spec.zv, spec.dv, spec.B, spec.H),
              aq_q=mk(spec.dq, spec.zq, 8, spec.qsym), aq_k=mk(spec.dk, spec.zk, 8, spec.qsym), aq_v=mk(spec.dv, spec.zv, 8, spec.qsym),
              aq_w=mk(spec.dw, spec.zpw, spec.wbits, spec.wsym), scale=spec.scale, prescale=spec.prescale,
              qc=qc, kc=kc, vc=vc, I=ev.I, want=want, decided=ev.decided, tol=ev.tol, ev=ev, pow2=pow2,
              features=sorted(set(features)), note=note, stated_undecided=stated_undecided, forms=spec.forms)
    return case


# ------------------------------------------------------------------------------------------------------------------------
# designed rows
# ------------------------------------------------------------------------------------------------------------------------
def designed(spec, rows, vfix=None, signature="auto"):
    """rows(bh, i) -> [(key, weight), ...]: query i of head bh scores weight * KM on each listed key (plus cross-talk of
    shared signature dims, which is exact like everything else).  vfix: {key: v code}."""
    rng, BH, T, S, d = spec.rng, spec.BH, spec.T, spec.S, spec.d
    qlo, qhi = spec.tilde_range(spec.zq)
    klo, khi = spec.tilde_range(spec.zk)
    KM = min(127, khi)
    nd = max(4, d // 2)                                       # design dims
    plan = [[rows(bh, i) for i in range(T)] for bh in range(BH)]
    live = sorted({j for hp in plan for r in hp for j, _ in r})
    if signature == "auto":
        signature = "onehot" if len(live) <= nd else "grid"
    if signature == "onehot":
        dims = {j: [n] for n, j in enumerate(live)}
    else:
        W = int(math.ceil(math.sqrt(S)))
        assert W + (S + W - 1) // W <= nd, (spec.name, S, nd)
        dims = {j: [j // W, (S + W - 1) // W + j % W] for j in live}
    kt = np.zeros((BH, S, d), dtype=np.int64)
    qt = np.zeros((BH, T, d), dtype=np.int64)
    for j, dd in dims.items():
        kt[:, j, dd] = KM

    def design_row(bh, i, nudge):
        row = np.zeros(nd, dtype=np.int64)
        for n, (j, w) in enumerate(plan[bh][i]):
            row[dims[j]] += w if n == 0 else max(0, w - nudge * n)
        qt[bh, i, :nd] = np.clip(row, qlo, qhi)
    for bh in range(BH):
        for i in range(T):
            design_row(bh, i, 0)
    # filler dims: random codes against the other side's zero point
    rest = np.arange(nd, d)
    r1, r2 = rest[: len(rest) // 2], rest[len(rest) // 2:]
    qt[:, :, r1] = rng.integers(qlo, qhi + 1, size=(BH, T, len(r1)))
    kt[:, :, r2] = rng.integers(klo, khi + 1, size=(BH, S, len(r2)))
    vc = rng.integers(spec.qmin, spec.qmax + 1, size=(BH, S, d))
    for j, code in (vfix or {}).items():
        vc[:, j, :] = code
    # rows that are not decided: lower the weights of their secondary keys by one more step (bounded)
    for nudge in range(1, REDRAWS + 1):
        bad = np.argwhere(~evaluate(spec, qt + spec.zq, kt + spec.zk, vc).decided)
        if not len(bad) or S * T > 200000:
            break
        for bh, i in bad:
            design_row(bh, i, nudge)
    return qt + spec.zq, kt + spec.zk, vc


def dense(spec, amp_q=24, amp_k=24):
    """Random small q~, k~ on every dim; undecided rows get their query redrawn."""
    rng, BH, T, S, d = spec.rng, spec.BH, spec.T, spec.S, spec.d
    qlo, qhi = spec.tilde_range(spec.zq)
    klo, khi = spec.tilde_range(spec.zk)
    draw = lambda lo, hi, amp, size: rng.integers(max(lo, -amp), min(hi, amp) + 1, size=size)
    kc = draw(klo, khi, amp_k, (BH, S, d)) + spec.zk
    qc = draw(qlo, qhi, amp_q, (BH, T, d)) + spec.zq
    vc = rng.integers(spec.qmin, spec.qmax + 1, size=(BH, S, d))
    for _ in range(REDRAWS):
        bad = ~evaluate(spec, qc, kc, vc).decided
        if not bad.any():
            break
        qc[bad] = draw(qlo, qhi, amp_q, (int(bad.sum()), d)) + spec.zq
    return qc, kc, vc


def all_rows(spec):
    return [(bh, i) for bh in range(spec.BH) for i in range(spec.T)]


# ------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------
GEOM_S = (1, 15, 16, 17, 31, 32, 33, 63, 65, 77)
GEOM_T = (1, 31, 33, 129)


def case_geometry(S, T, d=40, seed=0):
    """One-hot rows: query i puts nearly all mass on key (i + bh) mod S, a second live key sits at S - 1 (5 octaves below);
    every other key lies >= 45 octaves below.  A coarse 16-bit grid (dw = 2^-10) keeps the top code (~1000) decided although
    the maximum rises by up to 90 octaves after tile 0.  T = 129: the second block of 128 has one live row in one live wave."""
    spec = Spec(f"geom_S{S}_T{T}_d{d}", 2, 3, T, S, d, dw=2.0 ** -10, cs=2.0 ** -9, seed=seed)
    rows = lambda bh, i: [((i + bh) % S, 127), (S - 1, 120)]
    qc, kc, vc = designed(spec, rows, signature="grid")
    return finish(spec, qc, kc, vc, all_rows(spec), "one-hot rows over every key position")


def case_form(d, qsym, wbits, seed):
    """Dense random rows for one launch form: attn_kernel<d/32> (sym / asym, P8 / P16), the lean kernels for d = 24, 40, 80."""
    S = 45
    cs = 2.0 ** -9 / (2 if d > 128 else 1)
    dw = 2.0 ** -(8 if wbits == 8 else 12)
    spec = Spec(f"form_d{d}_{'sym' if qsym else 'asym'}_p{wbits}", 1, 2, 33, S, d, wbits=wbits, dw=dw, qsym=qsym, cs=cs,
                seed=seed)
    amp = max(6, int(24 * (32.0 / d) ** 0.5))
    qc, kc, vc = dense(spec, amp, amp)
    return finish(spec, qc, kc, vc, all_rows(spec), "dense random rows")


def case_scale_prescale():
    """A `scale` that is no power of two (fp32(40^-1/2) scaled so that cs stays exact) and a prescale of 1/2."""
    scale = float(np.float32(40 ** -0.5))
    spec = Spec("form_d40_scale_prescale", 2, 3, 33, 45, 40, dw=2.0 ** -12, cs=2.0 ** -8 * scale, scale=scale, prescale=0.5, seed=71)
    qc, kc, vc = dense(spec, 20, 20)
    return finish(spec, qc, kc, vc, all_rows(spec), "non power-of-two scale, prescale 1/2")


def case_zq_fallback(d):
    """q >= 0: the q zero point is code 0, stored -128, so -zq' = 128 does not fit one operand byte (c1 / c2 constants)."""
    S = 77 if d >= 40 else 61
    spec = Spec(f"zq-128_d{d}", 2, 3, 40, S, d, dw=2.0 ** -10, zq=0, cs=2.0 ** -9, seed=80 + d)
    rows = lambda bh, i: [((5 * i + bh) % S, 127), (S - 1, 118)]
    qc, kc, vc = designed(spec, rows, signature="grid")
    return finish(spec, qc, kc, vc, all_rows(spec), "stored q zero point -128")


def case_saturated(d, zq, zk, zv, seed):
    """Every operand code is an end code (0 or 255), zero points 0 / 255: |q~|, |k~|, |v~| = 255 wherever non-zero, so the
    scores of the kernel's own sum_d q~ k' reach d * 255 * 128.  Query 0 is all-far-end against one key that is all-far-end
    (and one that is all-near-end): a one-hot row of the top code on v = 255."""
    S, T = 24, 33
    cs = 2.0 ** -17 * (256.0 / d if d < 256 else 1.0)
    cs = 2.0 ** round(math.log2(cs))
    spec = Spec(f"sat_d{d}_zq{zq}_zk{zk}_zv{zv}", 1, 2, T, S, d, dw=2.0 ** -16, zq=zq, zk=zk, zv=zv, cs=cs, seed=seed)
    rng = spec.rng
    ends = lambda size: 255 * rng.integers(0, 2, size=size)
    kc, vc = ends((spec.BH, S, d)), ends((spec.BH, S, d))
    qc = ends((spec.BH, T, d))
    qc[:, 0, :] = 255 - zq                                     # q~ = +-255 on every dim
    kc[:, S - 1, :] = 255 - zk                                 # the key that matches it: the row maximum, in the ragged tail
    kc[:, 3, :] = zk                                           # k~ = 0
    kc[:, 4, :] = 255 - zk
    kc[:, 4, : d // 2] = zk
    vc[:, [3, S - 1], :] = 255 - zv                            # |v~| = 255 on the keys that can be row 0's maximum
    for _ in range(REDRAWS):
        bad = ~evaluate(spec, qc, kc, vc).decided
        bad[:, 0] = False
        if not bad.any():
            break
        qc[bad] = ends((int(bad.sum()), d))
    return finish(spec, qc, kc, vc, [(bh, 0) for bh in range(spec.BH)], "end codes on q, k and v")


def case_epilogue_flat(name, dw, S, wbits=16, wsym=False, zpw=0, note=""):
    """Equal scores (q~ = 0) against v = 255, zv = 0: every key has p = 1/S."""
    spec = Spec(name, 1, 2, 33, S, 40, wbits=wbits, wsym=wsym, zpw=zpw, dw=dw, zv=0, cs=2.0 ** -9, seed=5)
    qc = np.full((spec.BH, spec.T, spec.d), spec.zq, dtype=np.int64)
    kc = spec.rng.integers(0, 256, size=(spec.BH, S, spec.d))
    vc = np.full((spec.BH, S, spec.d), 255, dtype=np.int64)
    vc[:, :, 1::2] = spec.rng.integers(0, 256, size=(spec.BH, S, spec.d // 2))
    return finish(spec, qc, kc, vc, all_rows(spec), note)


def case_epilogue_p8(name, wsym, zpw, dw):
    """8-bit probability grids: a non-zero zpw, and the symmetric grid [-128, 127] as CIFAR runs it (ubias = 128)."""
    spec = Spec(name, 2, 3, 40, 50, 40, wbits=8, wsym=wsym, zpw=zpw, dw=dw, cs=2.0 ** -9, seed=9)
    rows = lambda bh, i: [((3 * i + bh) % 50, 127), (49, 124), ((i + 7) % 50, 122)] if i else [(11, 127)]
    qc, kc, vc = designed(spec, rows, vfix={11: 255})
    return finish(spec, qc, kc, vc, all_rows(spec), "8-bit probability grid")


def _flat_rows(n):
    """n equal live keys, both half-waves of tile 0 first (keys 0, 4, 1, 5, ...)."""
    order = [0, 4, 1, 5, 2, 6, 3, 7]
    return (order + list(range(8, n)))[:n] if n > 8 else order[:n]


def case_bytes():
    """P16, dw = 2^-16: rows of n equal live keys (p = 1/n) whose largest code is 255 (n = 257), 256 (256), 257 (255),
    32768 (2), above the grid (1: c = 65536, clamped) and, with helper keys far below, 32767 and 65535.  Block 0 of 128
    queries has exactly ONE hi-live row (row 5: n = 2) among hi-dead ones (n = 257), so has its wave; block 1 is hi-dead
    (n = 300: the lo-only kernel of the LDS path); block 2 holds the other feature rows."""
    S, T = 320, 288
    spec = Spec("bytes_p16", 1, 2, T, S, 40, dw=2.0 ** -16, cs=2.0 ** -9, zv=0, seed=21)
    # group signatures: one dim per group size, key j carries it when it is one of the first n of _flat_rows
    groups = [257, 256, 255, 300, 2, 1]
    nd = len(groups)
    KM = 115                                                   # khi = 255 - zk = 115
    kt = np.zeros((spec.BH, S, spec.d), dtype=np.int64)
    for g, n in enumerate(groups):
        kt[:, _flat_rows(n), g] = KM
    # helper keys for 32767 and 65535: key 100 / 101 carry their own dims at a searched magnitude
    kt[:, 100, nd] = KM
    kt[:, 101, nd + 1] = KM
    qt = np.zeros((spec.BH, T, spec.d), dtype=np.int64)
    group_of = {}
    for i in range(T):
        if i < 128:
            g = 4 if i == 5 else 0
        elif i < 256:
            g = 3
        else:
            g = (i - 256) % len(groups)
        group_of[i] = g
        qt[:, i, g] = 127
    feats = [(bh, i) for bh in range(spec.BH) for i in [5, 4, 6, 127, 128, 255] + list(range(256, 256 + len(groups)))]
    # 32767: two equal keys (group n = 2) and helper 100 at weight w; 65535: one key (n = 1) and helper 101
    rest = np.arange(nd + 2, spec.d)
    r1, r2 = rest[: len(rest) // 2], rest[len(rest) // 2:]
    qlo, qhi = spec.tilde_range(spec.zq)
    klo, khi = spec.tilde_range(spec.zk)
    qt[:, :, r1] = spec.rng.integers(qlo, qhi + 1, size=(spec.BH, T, len(r1)))
    kt[:, :, r2] = spec.rng.integers(klo, khi + 1, size=(spec.BH, S, len(r2)))
    vc = spec.rng.integers(0, 256, size=(spec.BH, S, spec.d))
    vc[:, [0, 4], :] = 255
    qc, kc = qt + spec.zq, kt + spec.zk
    for row, g, hdim, target in ((270, 4, nd, 32767), (271, 5, nd + 1, 65535)):
        best = None
        for w in range(0, 128):
            qc[:, row, :nd + 2] = spec.zq
            qc[:, row, g] = spec.zq + 127
            qc[:, row, hdim] = spec.zq + w
            ev = evaluate(spec, qc[:, row:row + 1], kc, vc)
            top = int(ev.pu.max())
            if top == target and ev.decided.all():
                slack = float((np.abs(ev.c - np.floor(ev.c) - 0.5) - ev.m).min())
                if best is None or slack > best[0]:
                    best = (slack, w)
        assert best is not None, (row, target)
        qc[:, row, hdim] = spec.zq + best[1]
        feats += [(bh, row) for bh in range(spec.BH)]
    return finish(spec, qc, kc, vc, feats, "byte boundaries of the 16-bit codes, one hi-live row per wave / block")


def case_dynamics():
    """Row-maximum dynamics on the lean family (S = 77, d = 40, cs = 2^-8: a signature match is 90 octaves):
    row 0: the maximum is the last key of the ragged tail;  rows 1..: the maximum sits in tile 1 or 2 and tile 0 holds nothing
    within 90 octaves (the repeat pass);  row 8: all scores equal;  every dead key underflows exp2 (180 octaves below)."""
    spec = Spec("dynamics_S77", 2, 3, 40, 77, 40, dw=2.0 ** -10, cs=2.0 ** -8, seed=31)

    def rows(bh, i):
        if i == 0:
            return [(76, 127), (2, 125)]
        if i == 8:
            return []
        return [(32 + (7 * i + bh) % 45, 127), (76, 125)]
    qc, kc, vc = designed(spec, rows, signature="grid")
    qc[:, 8, :] = spec.zq
    return finish(spec, qc, kc, vc, all_rows(spec), "maximum in the tail / rising > 64 octaves / equal scores / exp2 underflow")


def case_dense_long():
    """S = 4096, T = 160, d = 40, P16, flat rows: only the per-row bound applies (stated: mean undecided keys per row)."""
    spec = Spec("dense_long_4096", 1, 2, 160, 4096, 40, dw=2.0 ** -20, cs=2.0 ** -13, seed=41)
    rng = spec.rng
    qlo, qhi = spec.tilde_range(spec.zq)
    klo, khi = spec.tilde_range(spec.zk)
    qc = rng.integers(-24, 25, size=(spec.BH, spec.T, spec.d)) + spec.zq
    kc = rng.integers(-24, 25, size=(spec.BH, spec.S, spec.d)) + spec.zk
    vc = rng.integers(0, 256, size=(spec.BH, spec.S, spec.d))
    return finish(spec, qc, kc, vc, [], "dense long rows", stated_undecided=True)


def case_sparse_long():
    """The sparse twin: live keys in tile 0 (both 16-key halves, positions 15 / 16 / 31), tile 1 (32), the last tiles
    (4064 = tile 127, 4094, 4095: the key-term table's last entries); every other key 45 octaves below."""
    spec = Spec("sparse_long_4096", 1, 2, 160, 4096, 40, dw=2.0 ** -9, cs=2.0 ** -9, seed=43)
    live = [0, 5, 15, 16, 31, 32, 2047, 4064, 4094, 4095]

    def rows(bh, i):
        a = live[(i + bh) % len(live)]
        b = live[(3 * i + 1) % len(live)]
        c = live[(7 * i + 2) % len(live)]
        return [(a, 127), (b, 124), (c, 121)]
    qc, kc, vc = designed(spec, rows, signature="onehot")
    return finish(spec, qc, kc, vc, all_rows(spec), "sparse long rows")


def build_cases():
    cases = []
    for n, S in enumerate(GEOM_S):
        cases.append(lambda S=S, n=n: case_geometry(S, 129, seed=n))
    for S in (33, 77):
        for T in (1, 31, 33):
            cases.append(lambda S=S, T=T: case_geometry(S, T, seed=S + T))
    n = 0
    for d in (32, 64, 96, 128, 160, 256, 24, 40, 80):
        for qsym in (False, True):
            for wbits in (16, 8):
                n += 1
                cases.append(lambda d=d, qsym=qsym, wbits=wbits, n=n: case_form(d, qsym, wbits, 100 + n))
    cases.append(case_scale_prescale)
    cases.append(lambda: case_zq_fallback(40))
    cases.append(lambda: case_zq_fallback(32))
    cases.append(lambda: case_zq_fallback(80))
    for d in (256, 80, 60):
        cases.append(lambda d=d: case_saturated(d, 0, 0, 0, 200 + d))
        cases.append(lambda d=d: case_saturated(d, 255, 255, 255, 300 + d))
    cases.append(lambda: case_saturated(256, 0, 255, 0, 400))
    cases.append(lambda: case_epilogue_flat("epi_dw2^-24_S160_clamped", 2.0 ** -24, 160,
                                            note="every code clamps at 65535: I = 160 * 65535 * 255 > 2^31, 64-bit epilogue only"))
    cases.append(lambda: case_epilogue_flat("epi_dw2^-23_S256", 2.0 ** -23, 256, note="first grid past the `small` threshold: codes 32768, I just below 2^31"))
    cases.append(lambda: case_epilogue_flat("epi_dw2^-22_S128_small", 2.0 ** -22, 128,
                                            note="finest power-of-two dw with `small`: code sum 2^22, 32-bit epilogue"))
    cases.append(lambda: case_epilogue_p8("epi_p8_zpw3", False, 3, 2.0 ** -8))
    cases.append(lambda: case_epilogue_p8("epi_p8_sym_cifar", True, 0, float(np.float32(1.0 / 127.0))))
    cases.append(case_bytes)
    cases.append(case_dynamics)
    cases.append(case_dense_long)
    cases.append(case_sparse_long)
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
# the criterion (shared by the host test, which applies it to planted mistakes, and the GPU test)
# ------------------------------------------------------------------------------------------------------------------------
def check_rows(case, got):
    """got: float32 [BH, T, d].  Returns (ok, report): decided rows within 1 fp32 ulp of float32(I) * float32(dw*dv) (bit-exact
    when dw and dv are powers of two), other rows within the undecided-key bound + 1 ulp."""
    got = np.asarray(got, dtype=np.float32)
    want = case.want
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    one = ulp32(want)
    dec = case.decided[:, :, None]
    if case.pow2:
        bad_dec = dec & (got != want)
    else:
        bad_dec = dec & ~(err <= one)
    lim = case.tol + one
    bad_und = ~dec & ~(err <= lim)
    und_rows = ~case.decided
    ratio = float((err / lim)[np.broadcast_to(~dec, err.shape)].max()) if und_rows.any() else 0.0
    rep = NS(decided_rows=int(case.decided.sum()), rows=int(case.decided.size), bad_decided=int(bad_dec.sum()),
             bad_undecided=int(bad_und.sum()), worst_undecided_ratio=ratio,
             first_bad=(tuple(int(x) for x in np.argwhere(bad_dec | bad_und)[0]) if (bad_dec | bad_und).any() else None))
    return rep.bad_decided == 0 and rep.bad_undecided == 0, rep


def old_criterion(got, want_int):
    """The statistical criterion of test_attention_fused, for the report only: <= 1 % of outputs beyond 2e-4 * range, none
    beyond 2e-2 * range."""
    got = np.asarray(got, dtype=np.float64)
    rng = np.abs(want_int).max()
    diff = np.abs(got - want_int)
    return bool((diff > 2e-4 * rng).mean() <= 1e-2 and diff.max() <= 2e-2 * rng)
