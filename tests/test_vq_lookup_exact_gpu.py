"""qd_vq_lookup on the GPU where its result is known WITHOUT a tolerance (inputs of tests/vq_lookup_cases.py: every score is exact in
fp32, so the index of every pixel, ties included, is the first index of an integer minimum), where it must not depend on something
(the layout of z, a power-of-two scale, the neighbours of a pixel that holds no number), and the gates that route a call to it.

Every call goes through vq_lookup_cases._run: forced slice count, poisoned workspace, sentinel row, byte-checked output rows.
Each test prints the number of pixel indices it compared exactly (profiles/vq_lookup_exact.txt)."""
import random

import pytest
import torch

from test_vq_lookup_host import _lattice_vq, _vq_module
from vq_lookup_cases import (BF16, F16, F32, FORCED, LAYOUTS, MIN_SLICE, STAGE, _assert_nearest, _run, codes, distinct_codes, first_min, lattice,
                             pixel_rows, place, split_pixels, values)

pytestmark = pytest.mark.gpu

N_E = [1, 127, 128, 129, 511, 512, 513, 1025, 8192]
NAME = {F32: "fp32", F16: "fp16", BF16: "bf16"}


@pytest.fixture
def lib():
    from qdiff import hip
    lib = hip.load()
    yield lib
    lib.qd_vq_config(-1)


def _compared(n):
    print(f"[vq-exact] pixel indices compared exactly: {n}")


def _ldo(T, dtype, extra):
    chunk = 4 if dtype == F32 else 8
    return (-(-T // chunk) + extra) * chunk


# ---- 2. exact rows -----------------------------------------------------------------------------------------------------------
def _draws(n=18):
    """a seeded subset of the product: every axis is dealt out in full before it repeats, so every value appears"""
    rng = random.Random(20261126)
    axes = dict(E=list(range(1, 9)), dt=[F32, F16, BF16], layout=LAYOUTS, n_e=N_E, P=[1, 255, 1023, 1025, 2051], kind=["wide", "narrow"],
                out=[F32, F16, BF16], T=[None, 1, 5, 8], extra=[0, 1])
    cols = {name: rng.sample((vals * n)[:n], n) for name, vals in axes.items()}
    return [dict({name: cols[name][i] for name in axes}, seed=7000 + i) for i in range(n)]


@pytest.mark.parametrize("c", _draws(), ids=lambda c: f"e{c['E']}_{NAME[c['dt']]}_{c['layout']}_n{c['n_e']}_P{c['P']}_{c['kind']}_t{c['T']}_{NAME[c['out']]}")
def test_exact_rows(cuda, lib, c):
    E, n_e, P, kind = c["E"], c["n_e"], c["P"], c["kind"]
    g = torch.Generator().manual_seed(c["seed"])
    kz, ke = lattice(kind, P, E, g), codes(kind, n_e, E, g)
    want, many = first_min(kz, ke, counts=True)
    print(f"pixels with more than one exact minimiser: {(many > 1).float().mean().item():.3f}")
    if kind == "narrow" and n_e > 1:                                    # (one code is one minimiser)
        assert (many > 1).float().mean() > 0.5                          # ... so that the tie-breaking is what is tested
    z = place(values(kind, kz).to(c["dt"]), *split_pixels(P), c["layout"], cuda)
    cb = values(kind, ke).to(cuda)
    table = None if c["T"] is None else torch.randn(n_e, c["T"], generator=g).to(cuda)
    ldo = _ldo(c["T"] or E, c["out"], c["extra"])
    for s in FORCED:
        assert torch.equal(_run(lib, cuda, z, cb, table, c["out"], ldo, s).cpu().long(), want), s
    _compared(len(FORCED) * P)


@pytest.mark.parametrize("n_e,E", [(n, E) for n in N_E for E in (1, 3, 7, 8) if E > 1 or n <= 129], ids=lambda v: str(v))
def test_every_code_position_wins(cuda, lib, n_e, E):
    """z = the codebook's own pairwise distinct rows: pixel j is at distance 0 from code j alone, so every record of every stage
    of every slice, the four-record tail included, must be scanned (once: a second visit could not change a strict minimum, a
    missed one leaves another index)"""
    ke = distinct_codes(n_e, E)
    rows = values("wide", ke)
    z, cb = place(rows, *split_pixels(n_e), "nchw", cuda), rows.to(cuda)
    for s in FORCED:
        assert torch.equal(_run(lib, cuda, z, cb, None, F32, _ldo(E, F32, 0), s).cpu().long(), torch.arange(n_e)), s
    _compared(len(FORCED) * n_e)


def test_ties_across_the_split(cuda, lib):
    """equal scores in different slices / stages: the lower index wins whichever slice holds it.  Pairs at the distances of the
    slices of every forced count (128: the policy and the most; 4096: two) and of an LDS stage (512: one slice)"""
    n_e, far = 8192, torch.tensor([0, 120, 120])
    pairs = [(0, MIN_SLICE), (MIN_SLICE - 1, 2 * MIN_SLICE - 1), (5, 5 + STAGE), (STAGE - 1, 2 * STAGE - 1), (1, 4097), (4095, 8191)]
    kz = torch.tensor([[10 * i - 30, 0, 0] for i in range(len(pairs))])
    ke = far.repeat(n_e, 1)
    for i, (a, b) in enumerate(pairs):
        ke[a], ke[b] = kz[i] + torch.tensor([3, 0, 0]), kz[i] - torch.tensor([3, 0, 0])
    swapped = torch.cat([ke[n_e // 2:], ke[:n_e // 2]])
    want, want_swapped = first_min(kz, ke), first_min(kz, swapped)
    assert want.tolist() == [a for a, _ in pairs] and want_swapped.tolist() == [min((a + 4096) % n_e, (b + 4096) % n_e) for a, b in pairs]
    assert first_min(kz, ke, counts=True)[1].tolist() == [2] * len(pairs)
    z = place(values("wide", kz), 1, 1, len(pairs), "nchw", cuda)
    one = place(values("wide", kz[:1] + 3), 1, 1, 1, "nchw", cuda)
    for s in FORCED:
        assert _run(lib, cuda, z, values("wide", ke).to(cuda), None, F32, 4, s).tolist() == want.tolist(), s
        assert _run(lib, cuda, z, values("wide", swapped).to(cuda), None, F32, 4, s).tolist() == want_swapped.tolist(), s
        assert _run(lib, cuda, z, values("wide", ke[:1]).repeat(n_e, 1).to(cuda), None, F32, 4, s).tolist() == [0] * len(pairs), s   # one row 8192 times
        assert _run(lib, cuda, one, values("wide", ke[:1]).repeat(n_e, 1).to(cuda), None, F32, 4, s).tolist() == [0], s              # ... at score -|e|^2/2
    _compared(len(FORCED) * (3 * len(pairs) + 1))


# ---- 3. the result does not depend on where a pixel sits ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("E,n_e", [(3, 700), (6, 513), (8, 1025)])
def test_layouts_give_the_same_indices(cuda, lib, E, n_e, dtype):
    """1113 = 21 * 53 pixels (a full tile and 89) of randn values, as B = 1, 3 and 7 images whose S is no multiple of 256"""
    P = 1113
    g = torch.Generator().manual_seed(300 + E)
    rows = (torch.randn(P, E, generator=g) * 1.5).to(dtype)
    cb = torch.randn(n_e, E, generator=g).to(cuda)
    shape = {1: (1, 21, 53), 3: (3, 7, 53), 7: (7, 3, 53)}
    base = _run(lib, cuda, place(rows, *shape[1], "nchw", cuda), cb, None, F32, 8, -1)
    _assert_nearest(place(rows, *shape[1], "nchw", cuda), cb, base)
    n = 0
    for layout, B in [("nchw", 3), ("nchw", 7), ("cl", 1), ("cl", 3), ("row", 1), ("px", 1), ("chslice", 3), ("bstride", 3), ("bstride", 7),
                      ("offset", 7), ("hstride", 3), ("hstride", 1)]:
        z = place(rows, *shape[B], layout, cuda)
        whole = z._base.clone() if z._base is not None else z.clone()
        for s in (-1, 1):
            assert torch.equal(_run(lib, cuda, z, cb, None, F32, 8, s), base), (layout, B, s)
            n += P
        assert torch.equal(pixel_rows(z).cpu(), rows) and torch.equal(z._base if z._base is not None else z, whole), (layout, B)   # read only
    perm = torch.randperm(P, generator=g)
    assert torch.equal(_run(lib, cuda, place(rows[perm], *shape[3], "nchw", cuda), cb, None, F32, 8, -1).cpu(), base.cpu()[perm])
    if dtype != F32:                                                    # the same values widened: the same pixels
        assert torch.equal(_run(lib, cuda, place(rows.float(), *shape[3], "cl", cuda), cb, None, F32, 8, -1), base)
        n += P
    _compared(n + P)


@pytest.mark.parametrize("E,n_e", [(3, 700), (7, 513), (8, 1025)])
def test_power_of_two_scaling(cuda, lib, E, n_e):
    """(2^k z, 2^k codebook) scales h, every product and every partial sum by 4^k exactly while nothing leaves the normal range:
    the same comparisons, the same indices"""
    P = 1113
    g = torch.Generator().manual_seed(400 + E)
    rows, cb = torch.randn(P, E, generator=g) * 1.5, torch.randn(n_e, E, generator=g)
    mags = torch.cat([rows.flatten(), cb.flatten()]).double().abs()
    assert (mags[mags > 0].min().item() * 2.0 ** -24) ** 2 > 2.0 ** -100 and (E + 1) * (mags.max().item() * 2.0 ** 24) ** 2 < 2.0 ** 100
    base = _run(lib, cuda, place(rows, 3, 7, 53, "nchw", cuda), cb.to(cuda), None, F32, 8, -1)
    for k in (24, -24):
        for s in (-1, 1):
            got = _run(lib, cuda, place(rows * 2.0 ** k, 3, 7, 53, "nchw", cuda), (cb * 2.0 ** k).to(cuda), None, F32, 8, s)
            assert torch.equal(got, base), (k, s)
    _compared(4 * P)


# ---- 4. values that are no numbers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("E,dtype", [(3, F32), (5, F16), (8, BF16)], ids=["e3_fp32", "e5_fp16", "e8_bf16"])
def test_a_poisoned_pixel_leaves_its_lane_alone(cuda, lib, E, dtype, bad):
    """a lane holds pixels p, p + 256, p + 512, p + 768 of a tile, the first two and the last two as the halves of packed
    registers: one of the four holds no number in one channel, the other three (and every other pixel) keep their index"""
    P, n_e, lane = 1100, 600, 37
    g = torch.Generator().manual_seed(500 + E)
    rows = (torch.randn(P, E, generator=g) * 1.5).to(dtype)
    cb = torch.randn(n_e, E, generator=g).to(cuda)
    n = 0
    for s in (1, 2):
        clean = _run(lib, cuda, place(rows, 1, 1, P, "nchw", cuda), cb, None, F32, 8, s)
        for k in range(4):
            p = lane + 256 * k
            poisoned = rows.clone()
            poisoned[p, (k + 1) % E] = bad
            got = _run(lib, cuda, place(poisoned, 1, 1, P, "nchw", cuda), cb, None, F32, 8, s)
            keep = torch.arange(P, device=cuda) != p
            assert torch.equal(got[keep], clean[keep]), (s, k)
            assert 0 <= got[p].item() < n_e and (bad == bad or got[p].item() == 0), (s, k, got[p].item())   # NaN: index 0
            n += P - 1
    _compared(n)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("E", [3, 7, 8])
def test_a_codebook_row_that_holds_no_number_never_wins(cuda, lib, E, bad):
    """such a row scores NaN or +inf for a finite pixel (h = +inf or NaN; -z e adds +-inf or NaN) and loses every strict
    comparison; the scores of the other rows are the same bits as with a far finite row in its place, so every index is"""
    P, n_e, where = 1100, 1025, [0, 600, 1024]
    g = torch.Generator().manual_seed(600 + E)
    rows = torch.randn(P, E, generator=g) * 1.5
    cb_far = torch.randn(n_e, E, generator=g)
    cb_far[where] = 1000.0
    cb_bad = cb_far.clone()
    for i, j in enumerate(where):
        cb_bad[j] = cb_far[(j + 7) % n_e]                                # a row that WOULD win another row's pixels
        cb_bad[j, i % E] = bad
    z = place(rows, 1, 1, P, "nchw", cuda)
    for s in FORCED:
        far, got = _run(lib, cuda, z, cb_far.to(cuda), None, F32, 8, s), _run(lib, cuda, z, cb_bad.to(cuda), None, F32, 8, s)
        assert torch.equal(got, far), s
        assert not torch.isin(got.cpu(), torch.tensor(where, dtype=torch.int32)).any()
    _assert_nearest(z, cb_far, far)
    _compared(len(FORCED) * P)


# ---- 5. the gates ------------------------------------------------------------------------------------------------------------
def _outcome(f):
    try:
        return f()
    except (RuntimeError, IndexError, ValueError) as e:
        return type(e)


def _same(a, b):
    return a is b if isinstance(a, type) or isinstance(b, type) else (a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b))


def test_gate_truth_table(cuda, monkeypatch):
    """each rejecting row: the gate says no, the quantizer makes no hip.vq_lookup call and gives what it gives with the knob off
    (bits, or the same refusal where the composition itself cannot take the arguments)"""
    from qdiff import first_stage_hip as fh, hip
    calls = []
    monkeypatch.setattr(hip, "vq_lookup", lambda *a, _f=hip.vq_lookup, **k: (calls.append(sorted(k)), _f(*a, **k))[1])
    g = torch.Generator().manual_seed(9)

    def module(e_dim=3, **kw):
        m = _vq_module(e_dim=e_dim, zc=e_dim, **kw).to(cuda)
        return m.requires_grad_(False)

    def latent(e_dim=3, dtype=F32, shape=None):
        return torch.randn(shape or (2, e_dim, 5, 7), generator=g).to(dtype).to(cuda)

    trainable = module()
    trainable.quantize.embedding.weight.requires_grad_(True)
    half = module()
    half.quantize.embedding.weight.data = half.quantize.embedding.weight.data.half()
    on_cpu = module()
    on_cpu.quantize.embedding.weight.data = on_cpu.quantize.embedding.weight.data.cpu()
    # (name, module, z, knob, grad enabled, served)
    table = [
        ("served", module(), latent(), "hip", False, True),
        ("served-fp16", module(), latent(dtype=F16), "hip", False, True),
        ("served-frozen-under-grad", module(), latent(), "hip", True, True),
        ("served-trainable-without-grad", trainable, latent(), "hip", False, True),
        ("knob-off", module(), latent(), "library", False, False),
        ("z-requires-grad", module(), latent().requires_grad_(True), "hip", True, False),
        ("trainable-codebook", trainable, latent(), "hip", True, False),
        ("e_dim-9", module(9), latent(9), "hip", False, False),
        ("half-codebook", half, latent(dtype=F16), "hip", False, False),
        ("codebook-on-cpu", on_cpu, latent(), "hip", False, False),
        ("z-3d", module(), latent(shape=(2, 3, 35)), "hip", False, False),
        ("z-empty", module(), latent(shape=(0, 3, 5, 7)), "hip", False, False),
        ("z-fp64", module(), latent(dtype=torch.float64), "hip", False, False),
        ("z-channels", module(), latent(4), "hip", False, False),
    ]
    for name, m, z, knob, grad, served in table:
        with torch.set_grad_enabled(grad):
            monkeypatch.setattr(fh, "DECODER_VQ", "library")
            off = [_outcome(lambda: m.quantize.indices(z)), _outcome(lambda: m.quantize(z))]
            assert not calls
            monkeypatch.setattr(fh, "DECODER_VQ", knob)
            assert fh.vq_kernel_serves(m.quantize, z) == served, name
            assert fh.vq_rows_serve(m, z) == served, name
            on = [_outcome(lambda: m.quantize.indices(z)), _outcome(lambda: m.quantize(z))]
        if served:
            assert calls == [["indices"], ["out"]], name
            del calls[:]
            _assert_nearest(z, m.quantize.embedding.weight.detach(), on[0])
            assert torch.equal(on[1], m.quantize.get_codebook_entry(on[0], (z.shape[0], z.shape[2], z.shape[3], z.shape[1])))
        else:
            assert not calls and _same(on[0], off[0]) and _same(on[1], off[1]), name
            if name == "z-requires-grad":
                assert not isinstance(on[1], type) and on[1].dtype == F32
    # post_quant_conv: the fused head takes a plain 1x1 convolution of at most 8 outputs
    monkeypatch.setattr(fh, "DECODER_VQ", "hip")
    z = latent()
    with torch.no_grad():
        for name, pq, served in [("1x1", torch.nn.Conv2d(3, 4, 1), True), ("1x1-8", torch.nn.Conv2d(3, 8, 1, bias=False), True),
                                 ("3x3", torch.nn.Conv2d(3, 4, 3, padding=1), False), ("grouped", torch.nn.Conv2d(3, 3, 1, groups=3), False),
                                 ("9-outputs", torch.nn.Conv2d(3, 9, 1), False), ("linear", torch.nn.Linear(3, 4), False),
                                 ("on-cpu", None, False)]:
            m = module()
            m.post_quant_conv = pq.to(cuda) if pq is not None else torch.nn.Conv2d(3, 4, 1)
            m.post_quant_conv.requires_grad_(False)
            assert fh.vq_kernel_serves(m.quantize, z) and fh.vq_rows_serve(m, z) == served, name
    m = module()
    m.post_quant_conv.requires_grad_(True)
    with torch.enable_grad():
        assert not fh.vq_rows_serve(m, z) and fh.vq_kernel_serves(m.quantize, z)    # a trainable post_quant_conv under grad
    assert not calls


@pytest.mark.parametrize("variant", ["3x3", "grouped"])
def test_unserved_post_quant_conv_decodes_on_the_composition(cuda, monkeypatch, variant):
    """decode_first_stage(engine="hip") of the tiny VQ model on lattice values (exact: kernel and composition pick the same rows):
    with a post_quant_conv the fused head does not take, no call carries a table and the image is the knob-off image bit for bit"""
    from qdiff import first_stage_hip as fh, hip
    from qdiff.arch import first_stage as fs
    m, z = _lattice_vq()
    c = m.post_quant_conv.in_channels
    assert m.post_quant_conv.out_channels == c
    torch.manual_seed(1)
    m.post_quant_conv = torch.nn.Conv2d(c, c, 3, padding=1) if variant == "3x3" else torch.nn.Conv2d(c, c, 1, groups=c)
    m, z = m.to(cuda), z.to(cuda)
    calls = []
    monkeypatch.setattr(hip, "vq_lookup", lambda *a, _f=hip.vq_lookup, **k: (calls.append(sorted(k)), _f(*a, **k))[1])
    with torch.no_grad():
        monkeypatch.setattr(fh, "DECODER_VQ", "library")
        off = fs.decode_first_stage(m, z, 1.0, engine="hip")
        assert not calls
        monkeypatch.setattr(fh, "DECODER_VQ", "hip")
        on = fs.decode_first_stage(m, z, 1.0, engine="hip")
    assert calls == [["out"]] and torch.equal(on, off)


def test_set_decoder_vq_on_the_gpu_box(cuda):
    from qdiff import first_stage_hip as fh
    before = fh.DECODER_VQ
    try:
        m, z = _vq_module().to(cuda), torch.zeros(1, 3, 2, 2, device=cuda)
        with torch.no_grad():
            for s, served in (("hip", True), ("off", False), ("1", True), ("library", False), ("on", True), ("0", False), ("", False)):
                fh.set_decoder_vq(s)
                assert fh.vq_kernel_serves(m.quantize, z) == served, s
            with pytest.raises(ValueError):
                fh.set_decoder_vq("sdpa")
    finally:
        fh.DECODER_VQ = before
