"""CPU tests (no GPU) of the host side of qd_vq_lookup (csrc/vq_lookup.hip, qdiff/hip.py, qdiff/first_stage_hip.py).

1. tests/vq_lookup_emulator.py gives the exact integer first minimum on the lattice inputs of tests/vq_lookup_cases.py.
2. The slice rule (vq_choose) through the real library: qd_vq_lookup_form and qd_vq_lookup_ws_bytes are pure host.
3. Every refusal of qd_vq_lookup, in the order of the source, with fake aligned pointers.  Each call carries a breach, so none
   reaches a launch.  A call that a one-slice form would accept without a workspace cannot be sent here; that the workspace is
   asked for only when slices > 1 is shown by the same arguments being refused AT the workspace check under two slices and by the
   form / byte queries under one.
4. The refusals of the wrapper hip.vq_lookup that are raised before the library is touched, and the strides it hands over.
5. vq_folded_table on CPU modules; the bound is gamma_(e_dim+1) (|E| |W|^T + |b|) with the unit roundoff of fp32, any summation order.
6. The routes of VectorQuantizer and decode_first_stage on the emulator, the gates patched open (they ask for a GPU tensor)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import vq_lookup_emulator
from conv_form_util import FAKE
from golden_util import load_fixture
from test_first_stage import _build
from test_first_stage_hip import DECODER_TOL, ENGINE
from vq_lookup_cases import (BF16, F16, F32, LAYOUTS, MAX_SLICES, MIN_SLICE, TILE, codes, distinct_codes, first_min, lattice, pixel_rows, place,
                             split_pixels, values)

QF32, QF16, QBF16 = 0, 1, 2
DTYPES = [pytest.param(F16, id="fp16"), pytest.param(BF16, id="bf16")]


@pytest.fixture
def lib():
    from qdiff import hip
    handle = hip.load()
    handle.qd_vq_config(-1)
    yield handle
    handle.qd_vq_config(-1)


# ---- 1. the emulator on exact inputs -----------------------------------------------------------------------------------------
def test_the_case_builders():
    for n_e, E in ((1, 1), (129, 1), (255, 1), (8192, 2), (8192, 3), (8192, 7), (8192, 8), (513, 5)):
        k = distinct_codes(n_e, E)
        assert k.shape == (n_e, E) and k.abs().max() <= 127 and torch.unique(k, dim=0).shape[0] == n_e
    with pytest.raises(AssertionError):
        distinct_codes(257, 1)
    kz, ke = torch.tensor([[1, 0], [0, 0], [5, 5]]), torch.tensor([[9, 9], [1, 0], [0, 1], [1, 0], [-1, 0]])
    first, many = first_min(kz, ke, counts=True)
    assert first.tolist() == [1, 1, 0] and many.tolist() == [2, 4, 1]              # [0,0]: four codes of norm 1, the first is 1
    for P in (1, 255, 1023, 1025, 2051, 1113):
        B, H, W = split_pixels(P)
        assert B * H * W == P
    assert split_pixels(1023)[0] == 3 and split_pixels(2051)[0] == 7 and split_pixels(1025)[1] > 1
    rows = torch.arange(24.0).view(12, 2)
    for layout in LAYOUTS:
        z = place(rows, 2, 3, 2, layout, "cpu")
        assert torch.equal(pixel_rows(z), rows) and z.shape[1] == 2, layout
    assert not place(rows, 2, 3, 2, "hstride", "cpu").is_contiguous() and place(rows, 2, 3, 2, "offset", "cpu").storage_offset() == 7


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("kind", ["wide", "narrow"])
@pytest.mark.parametrize("E,n_e,P", [(1, 129, 300), (2, 513, 257), (3, 1025, 130), (5, 127, 64), (7, 512, 99), (8, 700, 131)])
def test_emulator_is_the_integer_first_minimum(kind, E, n_e, P, dtype):
    g = torch.Generator().manual_seed(5000 + E)
    kz, ke = lattice(kind, P, E, g), codes(kind, n_e, E, g)
    want, many = first_min(kz, ke, counts=True)
    if kind == "narrow":
        assert (many > 1).float().mean() > 0.5
    B, H, W = split_pixels(P)
    cb = values(kind, ke)
    z = place(values(kind, kz).to(dtype), B, H, W, LAYOUTS[(E + n_e) % len(LAYOUTS)], "cpu")
    assert torch.equal(pixel_rows(z).double() * (16 if kind == "wide" else 1), kz.double())      # the cast kept every value
    idx = torch.full((P + 1,), -7, dtype=torch.int32)
    out = torch.full((P + 1, 8), -1234.0, dtype=dtype)
    vq_lookup_emulator.vq_lookup(z, cb, indices=idx, out=out[:P])
    assert torch.equal(idx[:P].long(), want) and idx[P] == -7 and (out[P] == -1234.0).all()
    assert torch.equal(out[:P, :E], cb[want].to(dtype)) and (out[:P, E:] == 0).all()
    s = vq_lookup_emulator.vq_scores(pixel_rows(z), cb).double()                     # ... because its scores are the exact ones
    unit = 512 if kind == "wide" else 2
    assert torch.equal(s * unit, ((ke * ke).sum(1)[None] - 2 * kz @ ke.t()).double())


def test_emulator_on_values_that_are_no_numbers():
    cb = torch.tensor([[1.0, 1.0], [0.0, 2.0], [-1.0, 0.5], [3.0, -1.0]])
    nan, inf = float("nan"), float("inf")
    z = torch.tensor([[nan, 0.0], [0.0, 1.9], [inf, 0.0], [-inf, 0.0], [0.0, inf]]).t().reshape(1, 2, 1, 5).contiguous()
    idx = torch.empty(5, dtype=torch.int32)
    vq_lookup_emulator.vq_lookup(z, cb, indices=idx)
    # +inf in channel 0: rows with e_0 > 0 score -inf (the first is 0), e_0 = 0 scores NaN; -inf: row 2; channel 1: e_1 > 0 first at 0
    assert idx.tolist() == [0, 1, 0, 2, 0]
    for bad in (nan, inf, -inf):                                                    # such a codebook row never wins
        cb2 = cb.clone()
        cb2[1, 0] = bad
        vq_lookup_emulator.vq_lookup(z[..., 1:2], cb2, indices=idx[:1])
        assert idx[0].item() == 0                                                  # (1, 1) is next to (0, 1.9) once row 1 is out


# ---- 2. the rule through the real library ------------------------------------------------------------------------------------
PIXELS = [(1, 1), (1, 1024), (1024, 1), (5, 205), (255, 1024), (256, 1024), (1, (1 << 31) - 1), ((1 << 31) - 1, 1)]
CODES = [1, 127, 128, 129, 8191, 8192, 8193, 1 << 20]
KNOBS = [-1, 1, 2, 3, 63, 64, 65, 1 << 20]


def _form(lib, B, S, n_e):
    form = (ctypes.c_int32 * 2)(-1, -1)
    rc = lib.qd_vq_lookup_form(B, S, n_e, ctypes.cast(form, ctypes.c_void_p))
    return rc, tuple(form), lib.qd_last_error().decode()


@pytest.mark.parametrize("knob", KNOBS)
def test_the_slice_rule(lib, knob):
    lib.qd_vq_config(knob)
    for B, S in PIXELS:
        for n_e in CODES:
            P = B * S
            rc, (slices, launches), msg = _form(lib, B, S, n_e)
            assert rc == 0, msg
            tiles, most = -(-P // TILE), min(MAX_SLICES, -(-n_e // MIN_SLICE))
            want = knob if knob >= 1 else (1 if tiles >= 256 else -(-512 // tiles))
            want = max(1, min(want, most))
            per = -(--(-n_e // want) // MIN_SLICE) * MIN_SLICE
            where = (knob, B, S, n_e)
            assert 1 <= slices <= most, where
            assert slices == -(-n_e // per) and (slices - 1) * per < n_e, where    # no slice is empty
            if knob >= 1:
                assert slices <= knob, where
            elif tiles >= 256:
                assert slices == 1, where
            assert launches == (2 if slices > 1 else 1), where
            assert lib.qd_vq_lookup_ws_bytes(B, S, n_e) == (slices * P * 8 if slices > 1 else 0), where


def test_the_rule_at_the_points_the_design_names(lib):
    from qdiff import hip
    assert hip.vq_lookup_form(1, 4096, 8192) == (64, 2) and hip.vq_lookup_form(10, 4096, 8192) == (13, 2)
    assert hip.vq_lookup_form(16, 4096, 8192) == (8, 2) and hip.vq_lookup_form(64, 4096, 8192) == (1, 1)
    assert hip.vq_lookup_form(1, 65, MIN_SLICE) == (1, 1) and hip.vq_lookup_form(1, 65, 8192) == (64, 2)
    assert lib.qd_vq_lookup_ws_bytes(10, 4096, 8192) == 13 * 40960 * 8 and lib.qd_vq_lookup_ws_bytes(64, 4096, 8192) == 0
    lib.qd_vq_config(0)                                                             # anything below 1 is the policy
    assert hip.vq_lookup_form(1, 4096, 8192) == (64, 2)


@pytest.mark.parametrize("B,S,n_e", [(1, 1 << 31, 8192), (1 << 31, 1, 8192), (2, 1 << 30, 8192), (1 << 32, 1 << 32, 8192), (1 << 62, 4, 8192),
                                     (0, 64, 8192), (64, 0, 8192), (-1, 64, 8192), (64, -1, 8192), (1, 64, 0), (1, 64, -1), (1, 64, (1 << 20) + 1)])
def test_shapes_outside_the_contract(lib, B, S, n_e):
    rc, form, msg = _form(lib, B, S, n_e)
    assert rc != 0 and form == (-1, -1) and msg.startswith("qd_vq_lookup_form: need B, S >= 1"), msg
    assert lib.qd_vq_lookup_ws_bytes(B, S, n_e) == 0
    from qdiff import hip
    with pytest.raises(hip.HipEngineError, match="qd_vq_lookup_form"):
        hip.vq_lookup_form(B, S, n_e)


def test_form_needs_somewhere_to_write(lib):
    assert lib.qd_vq_lookup_form(1, 64, 8192, None) != 0 and "null form2" in lib.qd_last_error().decode()


# ---- 3. every refusal of qd_vq_lookup ----------------------------------------------------------------------------------------
# Arguments that pass every check but the last: 2 x 300 pixels, 256 codes under a knob of two slices (two of 128), no workspace.
BASE = dict(z=FAKE, z_dtype=QF32, B=2, S=300, e_dim=3, sb=900, sc=300, ss=1, codebook=FAKE, n_e=256, table=FAKE, t_dim=4, indices=FAKE,
            out=FAKE, out_dtype=QF16, ldo=8, ws=None, ws_bytes=0)
NEED = 2 * 600 * 8
AT_THE_WORKSPACE = "2 code slices need 9600 bytes of 8-byte aligned workspace"


def _call(lib, **kw):
    a = dict(BASE, **kw)
    rc = lib.qd_vq_lookup(a["z"], a["z_dtype"], a["B"], a["S"], a["e_dim"], a["sb"], a["sc"], a["ss"], a["codebook"], a["n_e"], a["table"], a["t_dim"],
                          a["indices"], a["out"], a["out_dtype"], a["ldo"], a["ws"], a["ws_bytes"], None)
    return rc, lib.qd_last_error().decode()


# (id, one or two breaches of BASE, substring of the refusal) in the order of the checks of the source
REFUSALS = [
    ("null-z", dict(z=None), "null z / codebook"),
    ("null-codebook", dict(codebook=None), "null z / codebook"),
    ("z-dtype-3", dict(z_dtype=3), "z_dtype must be f32/f16/bf16"),
    ("z-dtype-negative", dict(z_dtype=-1), "z_dtype must be f32/f16/bf16"),
    ("shape-B", dict(B=0), "need B, S >= 1"),
    ("shape-S", dict(S=-5), "need B, S >= 1"),
    ("shape-2^31", dict(B=1 << 16, S=1 << 15), "need B, S >= 1"),
    ("shape-n_e-0", dict(n_e=0), "need B, S >= 1"),
    ("shape-n_e-2^20+1", dict(n_e=(1 << 20) + 1), "need B, S >= 1"),
    ("e_dim-0", dict(e_dim=0), "e_dim 0 outside [1, 8]"),
    ("e_dim-9", dict(e_dim=9), "e_dim 9 outside [1, 8]"),
    ("z-misaligned-f32", dict(z=FAKE + 2), "z / codebook not aligned"),
    ("z-misaligned-f16", dict(z=FAKE + 1, z_dtype=QF16), "z / codebook not aligned"),
    ("z-misaligned-bf16", dict(z=FAKE + 1, z_dtype=QBF16), "z / codebook not aligned"),
    ("codebook-misaligned", dict(codebook=FAKE + 2), "z / codebook not aligned"),
    ("t_dim-0", dict(t_dim=0), "t_dim 0 outside [1, 8]"),
    ("t_dim-9", dict(t_dim=9, ldo=16), "t_dim 9 outside [1, 8]"),
    ("table-misaligned", dict(table=FAKE + 2), "(or table unaligned)"),
    ("no-output", dict(indices=None, out=None), "indices and out are both null"),
    ("indices-misaligned", dict(indices=FAKE + 2), "indices not 4-byte aligned"),
    ("out-dtype-3", dict(out_dtype=3), "out_dtype must be f32/f16/bf16"),
    ("ldo-short", dict(t_dim=8, ldo=0), "ldo must cover t_dim and be a multiple of 8"),
    ("ldo-short-f32", dict(out_dtype=QF32, t_dim=8, ldo=4), "ldo must cover t_dim and be a multiple of 4"),
    ("ldo-12-f16", dict(ldo=12), "ldo must cover t_dim and be a multiple of 8"),
    ("ldo-12-bf16", dict(out_dtype=QBF16, ldo=12), "ldo must cover t_dim and be a multiple of 8"),
    ("ldo-6-f32", dict(out_dtype=QF32, ldo=6), "ldo must cover t_dim and be a multiple of 4"),
    ("out-misaligned", dict(out=FAKE + 8), "out 16-byte aligned"),
    ("workspace-missing", dict(), AT_THE_WORKSPACE + " (qd_vq_lookup_ws_bytes), got 0"),
    ("workspace-bytes-without-a-pointer", dict(ws_bytes=1 << 40), AT_THE_WORKSPACE + " (qd_vq_lookup_ws_bytes), got 0"),
    ("workspace-short", dict(ws=FAKE, ws_bytes=NEED - 1), AT_THE_WORKSPACE + " (qd_vq_lookup_ws_bytes), got 9599"),
    ("workspace-misaligned", dict(ws=FAKE + 4, ws_bytes=1 << 40), AT_THE_WORKSPACE),
    # what the earlier checks let through arrives at the workspace check
    ("f32-rows-of-12-pass", dict(out_dtype=QF32, ldo=12), AT_THE_WORKSPACE),
    ("no-table-is-the-codebook", dict(table=None, t_dim=77), AT_THE_WORKSPACE),
    ("indices-alone-ignore-the-row-fields", dict(out=None, out_dtype=9, ldo=-3), AT_THE_WORKSPACE),
    ("rows-alone", dict(indices=None), AT_THE_WORKSPACE),
    ("f16-z-at-an-odd-element", dict(z=FAKE + 2, z_dtype=QF16), AT_THE_WORKSPACE),
    ("largest-shape", dict(B=1, S=(1 << 31) - 1, n_e=1 << 20), "2 code slices need 34359738352 bytes"),
    # two breaches at once: the earlier check reports
    ("order-null-before-dtype", dict(z=None, z_dtype=3), "null z / codebook"),
    ("order-dtype-before-shape", dict(z_dtype=3, B=0), "z_dtype must be f32/f16/bf16"),
    ("order-shape-before-e_dim", dict(n_e=0, e_dim=9), "need B, S >= 1"),
    ("order-e_dim-before-alignment", dict(e_dim=9, z=FAKE + 2), "e_dim 9 outside [1, 8]"),
    ("order-alignment-before-t_dim", dict(codebook=FAKE + 2, t_dim=9), "z / codebook not aligned"),
    ("order-t_dim-before-outputs", dict(t_dim=0, indices=None, out=None), "t_dim 0 outside [1, 8]"),
    ("order-outputs-before-indices", dict(indices=None, out=None, out_dtype=3), "indices and out are both null"),
    ("order-indices-before-out-dtype", dict(indices=FAKE + 2, out_dtype=3), "indices not 4-byte aligned"),
    ("order-out-dtype-before-ldo", dict(out_dtype=3, ldo=3), "out_dtype must be f32/f16/bf16"),
    ("order-ldo-before-workspace", dict(ldo=12, ws=FAKE + 4, ws_bytes=1 << 40), "ldo must cover t_dim"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_launcher_refuses(lib, case):
    _, breach, needle = case
    lib.qd_vq_config(2)
    rc, msg = _call(lib, **breach)
    assert rc != 0 and needle in msg and msg.startswith("qd_vq_lookup: "), msg


def test_the_workspace_is_asked_for_only_when_there_are_slices(lib):
    """BASE is refused AT the workspace check under two slices, so it passes every other one; under a knob of one, and under the
    policy for a shape whose tiles fill the chip, the same shape has one slice and needs no bytes, and the check reads
    `if (slices > 1)`.  (Sending that call would launch.)"""
    a = BASE
    lib.qd_vq_config(2)
    assert _form(lib, a["B"], a["S"], a["n_e"])[1] == (2, 2) and lib.qd_vq_lookup_ws_bytes(a["B"], a["S"], a["n_e"]) == NEED
    assert _call(lib)[0] != 0
    lib.qd_vq_config(1)
    assert _form(lib, a["B"], a["S"], a["n_e"])[1] == (1, 1) and lib.qd_vq_lookup_ws_bytes(a["B"], a["S"], a["n_e"]) == 0
    rc, msg = _call(lib, ws=FAKE + 4, ws_bytes=3, ldo=12)                            # the checks before it still hold at one slice
    assert rc != 0 and "ldo must cover t_dim" in msg
    lib.qd_vq_config(-1)
    assert _form(lib, 256, 1024, a["n_e"])[1] == (1, 1) and lib.qd_vq_lookup_ws_bytes(256, 1024, a["n_e"]) == 0


# ---- 4. the wrapper ----------------------------------------------------------------------------------------------------------
def _wrapper_args(**kw):
    a = dict(z=torch.zeros(2, 3, 4, 5), codebook=torch.zeros(16, 3), table=torch.zeros(16, 4), indices=torch.zeros(40, dtype=torch.int32),
             out=torch.zeros(40, 8, dtype=F16), ws=None)
    a.update(kw)
    return a


WRAPPER_REFUSALS = [
    ("z-3d", dict(z=torch.zeros(2, 3, 20)), "z must be a 4-d"),
    ("z-5d", dict(z=torch.zeros(1, 2, 3, 4, 5)), "z must be a 4-d"),
    ("z-int", dict(z=torch.zeros(2, 3, 4, 5, dtype=torch.int32)), "z must be a 4-d"),
    ("z-fp64", dict(z=torch.zeros(2, 3, 4, 5, dtype=torch.float64)), "z must be a 4-d"),
    ("codebook-strided", dict(codebook=torch.zeros(16, 6)[:, ::2]), "codebook must be a dense 2-d float32"),
    ("codebook-fp16", dict(codebook=torch.zeros(16, 3, dtype=F16)), "codebook must be a dense 2-d float32"),
    ("codebook-1d", dict(codebook=torch.zeros(48)), "codebook must be a dense 2-d float32"),
    ("codebook-channels", dict(codebook=torch.zeros(16, 4)), "does not match z's 3 channels"),
    ("table-strided", dict(table=torch.zeros(4, 16).t()), "table must be a dense 2-d float32"),
    ("table-bf16", dict(table=torch.zeros(16, 4, dtype=BF16)), "table must be a dense 2-d float32"),
    ("table-rows", dict(table=torch.zeros(15, 4)), "(or the table's rows)"),
    ("indices-short", dict(indices=torch.zeros(39, dtype=torch.int32)), "indices must be a dense int32"),
    ("indices-int64", dict(indices=torch.zeros(40, dtype=torch.int64)), "indices must be a dense int32"),
    ("indices-strided", dict(indices=torch.zeros(80, dtype=torch.int32)[::2]), "indices must be a dense int32"),
    ("out-strided", dict(out=torch.zeros(40, 16, dtype=F16)[:, :8]), "out must be dense"),
    ("out-short", dict(out=torch.zeros(39, 8, dtype=F16)), "out must be dense"),
    ("out-1d", dict(out=torch.zeros(320, dtype=F16)), "out must be dense"),
    ("out-int", dict(out=torch.zeros(40, 8, dtype=torch.int16)), "out must be dense"),
]


@pytest.mark.parametrize("case", WRAPPER_REFUSALS, ids=[r[0] for r in WRAPPER_REFUSALS])
def test_wrapper_refuses_before_the_library(monkeypatch, case):
    from qdiff import hip
    _, breach, needle = case

    def touched():
        raise AssertionError("the library was loaded for a refused call")
    monkeypatch.setattr(hip, "load", touched)
    with pytest.raises(hip.HipEngineError) as e:
        hip.vq_lookup(**_wrapper_args(**breach))
    assert needle in str(e.value) and str(e.value).startswith("vq_lookup: ")


class _Recorder:
    """stands where the library does: keeps the arguments of qd_vq_lookup, launches nothing"""

    def __init__(self):
        self.calls = []

    def qd_vq_lookup_ws_bytes(self, B, S, n_e):
        return 0

    def qd_vq_lookup(self, *a):
        self.calls.append(a)
        return 0


def _addressed(z, a):
    """the elements the kernel reads for the arguments `a` of one recorded call, as pixel rows: base + (p / S) sb + (p % S) ss + c sc"""
    _, _, B, S, E, sb, sc, ss = a[:8]
    flat = torch.as_strided(z, (z.untyped_storage().nbytes() // z.element_size(),), (1,), 0)
    p, c = torch.arange(B * S)[:, None], torch.arange(E)[None]
    off = (a[0] - flat.data_ptr()) // z.element_size() + (p // S) * sb + (p % S) * ss + c * sc
    assert 0 <= off.min() and off.max() < flat.numel(), "the kernel would read outside the tensor"
    return flat[off]


VIEWS = {
    "nchw": lambda x: x,
    "channels-last": lambda x: x.contiguous(memory_format=torch.channels_last),
    "channel-slice": lambda x: torch.cat([x, x, x], 1)[:, x.shape[1]:2 * x.shape[1]],
    "batch-strided": lambda x: torch.cat([x, x], 0)[::2] if x.shape[0] == 1 else torch.stack([x, -x], 1).flatten(0, 1)[::2],
    "width-strided": lambda x: torch.cat([x, x], 3)[..., :x.shape[3]],
    "height-strided": lambda x: torch.cat([x, x], 2)[:, :, ::2][:, :, :x.shape[2]],
    "transposed": lambda x: x.reshape(x.shape[0], x.shape[1], x.shape[3], x.shape[2]).transpose(2, 3),    # width-major storage
    "expanded": lambda x: x[:, :, :1, :1].expand_as(x),
}


@pytest.mark.parametrize("shape", [(2, 3, 4, 5), (2, 3, 5, 1), (1, 3, 5, 1), (1, 3, 1, 5), (3, 1, 1, 1), (1, 8, 1, 1), (2, 1, 3, 1)], ids=str)
@pytest.mark.parametrize("view", list(VIEWS))
def test_wrapper_hands_over_strides_that_address_the_pixels(monkeypatch, view, shape):
    """whatever strides torch keeps on axes of one element, the (pointer, sb, sc, ss) of the call address exactly z's pixels, in
    order, inside its storage; a view whose pixel axes do not collapse is copied and the caller's tensor stays as it was"""
    from qdiff import hip
    rec = _Recorder()
    monkeypatch.setattr(hip, "load", lambda: rec)
    monkeypatch.setattr(hip, "_stream", lambda: None)
    seen = {}
    monkeypatch.setattr(hip, "_ptr", lambda t, name=None: None if t is None else (seen.__setitem__(name, t), t.data_ptr())[1])
    z = VIEWS[view](torch.arange(1.0, 1 + torch.Size(shape).numel()).view(shape))
    before, strides = z.clone(), z.stride()
    B, E, H, W = shape
    hip.vq_lookup(z, torch.zeros(16, E), indices=torch.zeros(B * H * W, dtype=torch.int32))
    (a,) = rec.calls
    assert a[1:5] == (QF32, B, H * W, E) and a[9] == 16 and a[11] == E
    assert torch.equal(_addressed(seen["z"], a), pixel_rows(before))
    assert torch.equal(z, before) and z.stride() == strides


# ---- 5. the folded table -----------------------------------------------------------------------------------------------------
def _vq_module(bias=True, n_e=96, e_dim=3, zc=4, seed=3):
    from qdiff.arch import first_stage as fs
    torch.manual_seed(seed)
    m = torch.nn.Module()
    m.quantize = fs.VectorQuantizer(n_e, e_dim)
    m.post_quant_conv = torch.nn.Conv2d(e_dim, zc, 1, bias=bias)
    with torch.no_grad():
        m.quantize.embedding.weight.mul_(3.0)
    return m


def _post_quant_fp64(pq, x):
    """post_quant_conv evaluated in fp64 (the module itself is left alone: a cast would re-make its parameters)"""
    return F.conv2d(x.double(), pq.weight.detach().double(), None if pq.bias is None else pq.bias.detach().double())


def _assert_folded(m, t):
    e, pq = m.quantize.embedding.weight.detach(), m.post_quant_conv
    want = _post_quant_fp64(pq, e.t()[None, :, :, None])[0, :, :, 0].t()           # the embedding rows as 1x1 pixels
    w = pq.weight.detach().double().reshape(pq.out_channels, -1)
    n = e.shape[1] + 1
    gamma = n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
    bound = gamma * (e.double().abs() @ w.abs().t() + (pq.bias.detach().double().abs() if pq.bias is not None else 0.0))
    assert t.dtype == F32 and t.is_contiguous() and tuple(t.shape) == (e.shape[0], pq.out_channels)
    assert ((t.double() - want).abs() <= bound).all()


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no-bias"])
def test_folded_table_is_post_quant_conv_of_the_codebook(bias):
    from qdiff import first_stage_hip as fh
    for e_dim, zc in ((3, 4), (1, 1), (8, 8), (4, 3)):
        m = _vq_module(bias, e_dim=e_dim, zc=zc)
        t = fh.vq_folded_table(m)
        _assert_folded(m, t)
        assert fh.vq_folded_table(m) is t                                          # cached


@pytest.mark.parametrize("how", ["in-place", "re-assigned"])
@pytest.mark.parametrize("which", ["embedding", "weight", "bias"])
def test_folded_table_follows_its_parameters(which, how):
    from qdiff import first_stage_hip as fh
    m = _vq_module()
    t = fh.vq_folded_table(m)
    owner, name = {"embedding": (m.quantize.embedding, "weight"), "weight": (m.post_quant_conv, "weight"), "bias": (m.post_quant_conv, "bias")}[which]
    old = getattr(owner, name)
    if how == "in-place":
        with torch.no_grad():
            old.add_(0.75)
    else:
        setattr(owner, name, torch.nn.Parameter(old.detach() * 1.5 + 0.25))
    t2 = fh.vq_folded_table(m)
    assert t2 is not t and not torch.equal(t2, t)
    _assert_folded(m, t2)
    assert fh.vq_folded_table(m) is t2
    if which == "bias" and how == "re-assigned":                                   # and a bias taken away
        m.post_quant_conv.bias = None
        t3 = fh.vq_folded_table(m)
        assert t3 is not t2
        _assert_folded(m, t3)


def test_folded_table_follows_a_loaded_state_dict():
    from qdiff import first_stage_hip as fh
    m, other = _vq_module(seed=3), _vq_module(seed=4)
    t = fh.vq_folded_table(m)
    m.load_state_dict(other.state_dict())
    _assert_folded(m, fh.vq_folded_table(m))
    assert not torch.equal(fh.vq_folded_table(m), t)


# ---- 6. the routes on the emulator -------------------------------------------------------------------------------------------
@pytest.fixture
def route(monkeypatch):
    """(first_stage_hip, the keyword sets of the hip.vq_lookup calls): every launch wrapper on its emulator, the two gates open
    for CPU tensors while the knob says hip"""
    import abi_emulator
    from qdiff import first_stage_hip as fh, hip
    from qdiff.arch import first_stage as fs
    abi_emulator.install(monkeypatch)
    vq_lookup_emulator.install(monkeypatch)
    calls = []
    monkeypatch.setattr(hip, "vq_lookup", lambda *a, _f=hip.vq_lookup, **k: (calls.append(sorted(k)), _f(*a, **k))[1])
    monkeypatch.setattr(fh, "DECODER_VQ", "library")
    monkeypatch.setattr(fs.VectorQuantizer, "_hip", lambda self, z: fh if fh.DECODER_VQ == "hip" else None)
    monkeypatch.setattr(fh, "vq_rows_serve", lambda first_stage, z: fh.DECODER_VQ == "hip")
    return fh, calls


def _lattice_vq(seed=11):
    """the tiny VQ configuration with its codebook and a latent of its shape on the wide lattice"""
    case = load_fixture("first_stage.pt")["vq_tiny"]
    m = _build(case, "vq")
    g = torch.Generator().manual_seed(seed)
    n_e, e_dim = m.quantize.embedding.weight.shape
    b, _, h, w = case["z"].shape
    with torch.no_grad():
        m.quantize.embedding.weight.copy_(values("wide", lattice("wide", n_e, e_dim, g)) / 32)
    kz = lattice("wide", 2 * b * h * w, e_dim, g)
    return m, place(values("wide", kz) / 32, 2 * b, h, w, "nchw", "cpu")


def test_quantizer_routes_equal_the_composition(route):
    """on lattice values (here scaled by 2^-5 to the size of a latent, which changes nothing) the composition's fp32 distances are
    exact too, so its argmin is the same first minimum"""
    fh, calls = route
    m, z = _lattice_vq()
    with torch.no_grad():
        off_idx, off = m.quantize.indices(z), m.quantize(z)
        assert not calls
        fh.set_decoder_vq("hip")
        on_idx, on = m.quantize.indices(z), m.quantize(z)
    assert calls == [["indices"], ["out"]]
    assert on_idx.dtype == torch.int64 and on_idx.shape == (z.shape[0] * z.shape[2] * z.shape[3],) and torch.equal(on_idx, off_idx)
    assert on.dtype == F32 and on.shape == z.shape and on.is_contiguous() and torch.equal(on, off)
    ke = (m.quantize.embedding.weight.detach() * 512).round().long()
    assert torch.equal(on_idx, first_min((pixel_rows(z) * 512).round().long(), ke))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_head_feeds_conv_in_the_rows_of_the_composition(route, dtype):
    from qdiff.arch import first_stage as fs
    fh, calls = route
    m, z = _lattice_vq()
    hd = fh.hip_decoder(m.decoder, dtype)
    with torch.no_grad():
        exact = _post_quant_fp64(m.post_quant_conv, m.quantize(z))
        lib_out, ref = fs.decode_first_stage(m, z, 1.0, engine=ENGINE[dtype]), m.decode(z)
        assert not calls
        fh.set_decoder_vq("hip")
        rows = fh.vq_rows(m, z, hd)
        out = fs.decode_first_stage(m, z, 1.0, engine=ENGINE[dtype])
    assert calls == [["out", "table"], ["out", "table"]]
    b, _, h, w = z.shape
    zc = m.post_quant_conv.out_channels
    assert rows.dtype == dtype and tuple(rows.shape) == (b * h * w, hd.conv_in_width(z.device)) and (rows[:, zc:] == 0).all()
    # one fp32 evaluation of e_dim products, e_dim - 1 sums and the bias (gamma_(e_dim+1), any order), then ONE rounding to the
    # operand type: unit roundoff 2^-11 (fp16; its subnormal spacing 2^-24) or 2^-8 (bf16)
    want = pixel_rows(exact)
    e, pq = m.quantize.embedding.weight.detach().double(), m.post_quant_conv
    n = e.shape[1] + 1
    gamma = n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
    mag = pixel_rows(m.quantize(z).detach().double()).abs() @ pq.weight.detach().double().reshape(zc, -1).abs().t() + pq.bias.detach().double().abs()
    u = 2.0 ** -11 if dtype == F16 else 2.0 ** -8
    bound = u * want.abs() + (1 + u) * gamma * mag + (2.0 ** -25 if dtype == F16 else 0.0)
    assert ((rows[:, :zc].double() - want).abs() <= bound).all()
    err = (out - ref).abs().max().item() / ref.abs().max().item()
    assert out.shape == ref.shape and err <= DECODER_TOL[dtype], err
    assert (out - lib_out).abs().max().item() / ref.abs().max().item() <= DECODER_TOL[dtype]


def test_knob_strings():
    from qdiff import first_stage_hip as fh
    before = fh.DECODER_VQ
    try:
        for s, want in (("", "library"), (None, "library"), ("library", "library"), ("0", "library"), ("off", "library"), (" Library ", "library"),
                        ("OFF", "library"), ("hip", "hip"), ("1", "hip"), ("on", "hip"), (" HIP\n", "hip"), ("On", "hip")):
            fh.set_decoder_vq(s)
            assert fh.DECODER_VQ == want, s
        for s in ("sdpa", "2", "true", "hip,library", "triton", "-1"):
            fh.set_decoder_vq("hip")
            with pytest.raises(ValueError, match="QDIFF_DECODER_VQ"):
                fh.set_decoder_vq(s)
            assert fh.DECODER_VQ == "hip"                                          # a refused string changes nothing
    finally:
        fh.DECODER_VQ = before


def test_gates_on_the_host():
    """no GPU tensor, no kernel: the gate and VectorQuantizer._hip say no to every CPU tensor whatever the knob says"""
    from qdiff import first_stage_hip as fh
    m = _vq_module()
    before = fh.DECODER_VQ
    try:
        fh.set_decoder_vq("hip")
        z = torch.zeros(1, 3, 2, 2)
        assert not fh.vq_kernel_serves(m.quantize, z) and not fh.vq_rows_serve(m, z) and m.quantize._hip(z) is None
        assert not fh.vq_kernel_serves(m.quantize, None) and m.quantize._hip([1.0]) is None
    finally:
        fh.DECODER_VQ = before
