"""CPU tests (no GPU) of the weights-only contraction's plan (csrc/wq_h16.hip: plan_wq) through the real library:
qd_conv2d_wq_h16_form is the plan with the launch withheld, a pure host function, so descriptors carry fake pointers and shape
fields only (as tests/conv_form_util.py builds them for qd_conv2d_i8_form).

1. The slices of the form agree with the workspace query, under the policy and under qd_wq_h16_config.
2. A missing or short workspace falls back to the one pass silently; a misaligned one is refused only where it would be used.
3. The finalise pass is the vectorised form exactly under the launcher's condition.
4. Every refusal of the launcher, through the form query AND through qd_conv2d_wq_h16 itself (each is refused before any launch),
   and the order of the checks.  The qd_conv2d_wq_h16 half needs nothing of this change: it passes on a library built from the
   revision before the plan existed (QDIFF_HIP_LIB=<that library> pytest tests/test_wq_form_host.py -k launcher_refuses).
"""
import ctypes

import pytest

from conv_form_util import FAKE
from test_weight_only_splitk_host import FULL_GRID, GEGLU, ONE_STEP, SD_8x8, SD_8x8_SHORTCUT, TEMB

ODD = dict(B=2, H=5, W=7, Cout=48, k=3, clens=[136])          # 27 K-steps: uneven slices under a forced count
SHAPES = dict(SD_8x8=SD_8x8, SD_8x8_SHORTCUT=SD_8x8_SHORTCUT, FULL_GRID=FULL_GRID, GEGLU=GEGLU, ONE_STEP=ONE_STEP, TEMB=TEMB, ODD=ODD)
AMPLE = 1 << 40
F32, F16, BF16 = 0, 1, 2
EPI_GEGLU_H16 = 4


@pytest.fixture
def lib():
    from qdiff import hip
    handle = hip.load()
    handle.qd_wq_h16_config(-1)
    yield handle
    handle.qd_wq_h16_config(-1)


def _desc(B, H, W, Cout, k, clens, epilogue=0, stride=1, wbits=4, act=F16, out=F32):
    """A descriptor the launcher accepts: fake 16-byte aligned pointers, shape fields of one layer."""
    from qdiff import hip
    d = hip.ConvDesc()
    d.x = d.w = d.out = FAKE
    d.B, d.H, d.W, d.Cout = B, H, W, Cout
    d.Ho, d.Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    d.kh = d.kw = k
    d.stride, d.pad_t, d.pad_l = stride, k // 2, k // 2
    d.wbits, d.w_tiled, d.epilogue, d.nseg = wbits, 1, epilogue, len(clens)
    d.ldx = sum(clens)
    if epilogue == EPI_GEGLU_H16:
        d.ldo, d.out_dtype = Cout // 2, act                   # operand rows of the next layer
    else:
        d.ldo, d.out_dtype = Cout, out
    c0 = 0
    for i, c in enumerate(clens):
        d.seg[i].c0, d.seg[i].clen, d.seg[i].scale, d.seg[i].zw = c0, c, FAKE, FAKE
        c0 += c
    return d


def _lend(d, nbytes=AMPLE, ptr=FAKE):
    d.splitk_ws, d.splitk_ws_bytes = ptr, nbytes
    return d


def _form(lib, d, act=F16):
    """(return code, form4, message)"""
    out = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    rc = lib.qd_conv2d_wq_h16_form(ctypes.byref(d) if d is not None else None, act, out)
    return rc, tuple(out), lib.qd_last_error().decode()


def _accepted(lib, d, act=F16):
    rc, form, msg = _form(lib, d, act)
    assert rc == 0, msg
    return form


def _steps(dd):
    return sum(dd["k"] * dd["k"] * ((c + 63) // 64) for c in dd["clens"])


def _mn4(dd):
    return dd["B"] * dd["H"] * dd["W"] * dd["Cout"] * 4


# ---- 1. slices agree with the workspace query ------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [F32, F16], ids=["out-f32", "out-f16"])
@pytest.mark.parametrize("act", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("wbits", [4, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_slices_agree_with_the_workspace_query(lib, name, wbits, act, out):
    dd = SHAPES[name]
    geglu = dd.get("epilogue") == EPI_GEGLU_H16
    total = _steps(dd)
    for knob in (-1, 0, 3, 40):
        lib.qd_wq_h16_config(knob)
        d = _lend(_desc(wbits=wbits, act=act, out=out, **dd))
        ws = int(lib.qd_conv2d_wq_h16_splitk_ws_bytes(ctypes.byref(d)))
        assert ws % _mn4(dd) == 0
        slices, it_per, epi, vec = _accepted(lib, d, act)
        assert slices == (ws // _mn4(dd) if ws else 1), (name, knob)
        if slices >= 2:
            assert it_per == -(-total // slices) and -(-total // it_per) == slices, (name, knob)    # no slice is empty
        else:
            assert (it_per, vec) == (0, 0), (name, knob)
        assert epi == (2 if geglu else 1 if out == F16 else 0)
        if geglu or knob == 0:
            assert slices == 1
    lib.qd_wq_h16_config(-1)
    assert (_accepted(lib, _lend(_desc(**SD_8x8)))[0] >= 2 and _accepted(lib, _lend(_desc(**SD_8x8_SHORTCUT)))[0] >= 2)


# ---- 2. the fall-back is silent and exact ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SD_8x8", "SD_8x8_SHORTCUT", "ODD"])
def test_fallback_to_one_pass_is_silent_and_exact(lib, name):
    dd = SHAPES[name]
    if name == "ODD":
        lib.qd_wq_h16_config(4)                               # (the policy does not slice 27 K-steps)
    sliced = _accepted(lib, _lend(_desc(**dd)))
    need = sliced[0] * _mn4(dd)
    assert sliced[0] >= 2 and need == int(lib.qd_conv2d_wq_h16_splitk_ws_bytes(ctypes.byref(_desc(**dd))))
    assert _accepted(lib, _lend(_desc(**dd), need)) == sliced                    # exactly enough
    one_pass = (1, 0, 0, 0)
    assert _accepted(lib, _desc(**dd)) == one_pass                               # no workspace
    assert _accepted(lib, _lend(_desc(**dd), AMPLE, None)) == one_pass           # bytes without a pointer
    assert _accepted(lib, _lend(_desc(**dd), need - 1)) == one_pass              # one byte short
    assert _accepted(lib, _lend(_desc(out=F16, **dd), need - 1)) == (1, 0, 1, 0)


def test_misaligned_workspace_is_refused_only_where_it_is_used(lib):
    d = _lend(_desc(**SD_8x8), AMPLE, FAKE + 4)
    rc, _, msg = _form(lib, d)
    assert rc != 0 and "splitk_ws must be 16-byte aligned" in msg
    assert lib.qd_conv2d_wq_h16(ctypes.byref(d), F16, None) != 0                 # (refused before any launch)
    assert "splitk_ws must be 16-byte aligned" in lib.qd_last_error().decode()
    for dd in (FULL_GRID, ONE_STEP, TEMB, GEGLU):                                # not sliced: the pointer is never looked at
        assert _accepted(lib, _lend(_desc(**dd), AMPLE, FAKE + 4))[0] == 1
    assert _accepted(lib, _lend(_desc(**SD_8x8), 16, FAKE + 4))[0] == 1           # nor where the workspace is too small to use
    lib.qd_wq_h16_config(0)
    assert _accepted(lib, _lend(_desc(**SD_8x8), AMPLE, FAKE + 4))[0] == 1


# ---- 3. finalise form ------------------------------------------------------------------------------------------------------
def _full(out=F32):
    """SD_8x8 sliced, with bias, rowbias and residual: every operand of the finalise pass allows four columns per thread."""
    d = _lend(_desc(out=out, **SD_8x8))
    d.bias = d.rowbias = d.residual = FAKE
    d.ld_rowbias = d.ldr = d.ldo = d.Cout
    return d


@pytest.mark.parametrize("out", [F32, F16], ids=["out-f32", "out-f16"])
def test_finalise_is_vectorised_exactly_when_every_operand_allows(lib, out):
    base = _accepted(lib, _full(out))
    assert base[0] >= 2 and base[2] == out and base[3] == 1
    N = SD_8x8["Cout"]
    breaches = [dict(ldo=N + 2), dict(out=FAKE + 4), dict(bias=FAKE + 4), dict(rowbias=FAKE + 4), dict(ld_rowbias=N + 2),
                dict(residual=FAKE + 4), dict(ldr=N + 2), dict(Cout=N - 2)]
    if out == F32:
        breaches.append(dict(out=FAKE + 8))
        breaches.append(dict(residual=FAKE + 8))
    for b in breaches:
        d = _full(out)
        for k, v in b.items():
            setattr(d, k, v)
        form = _accepted(lib, d)
        assert form[:3] == base[:3] and form[3] == 0, b
    if out == F16:                                            # four fp16 elements are 8 bytes
        for b in (dict(out=FAKE + 8), dict(residual=FAKE + 8)):
            d = _full(out)
            for k, v in b.items():
                setattr(d, k, v)
            assert _accepted(lib, d) == base, b
    for absent in ("bias", "rowbias", "residual"):            # an absent operand constrains nothing
        d = _full(out)
        setattr(d, absent, None)
        assert _accepted(lib, d) == base, absent


# ---- 4. refusals: the table and the order ----------------------------------------------------------------------------------
def _linear(**kw):
    return _desc(**dict(dict(B=2, H=6, W=5, Cout=40, k=3, clens=[24]), **kw))


def _two_seg(**kw):
    return _linear(clens=[24, 16], **kw)


def _geglu(**kw):
    return _desc(**dict(dict(B=1, H=1, W=12, Cout=128, k=1, clens=[64], epilogue=EPI_GEGLU_H16), **kw))


def _set(d, **fields):
    for k, v in fields.items():
        if k.startswith("seg"):                               # seg0_clen -> d.seg[0].clen
            setattr(d.seg[int(k[3])], k[5:], v)
        else:
            setattr(d, k, v)
    return d


# (id, descriptor or None, act_dtype, substring of the refusal): one mutation of an accepted descriptor per QD_REQUIRE of plan_wq,
# in the order of the checks
REFUSALS = [
    ("null-descriptor", lambda: None, F16, "null descriptor"),
    ("null-x", lambda: _set(_linear(), x=None), F16, "null tensor pointer"),
    ("null-w", lambda: _set(_linear(), w=None), F16, "null tensor pointer"),
    ("null-out", lambda: _set(_linear(), out=None), F16, "null tensor pointer"),
    ("res-period", lambda: _set(_linear(), res_period=4), F16, "res_period is not supported"),
    ("act-f32", lambda: _linear(), F32, "act_dtype must be QD_F16 or QD_BF16"),
    ("not-tiled", lambda: _set(_linear(), w_tiled=0), F16, "weights must be tile-ordered codes"),
    ("wbits-5", lambda: _set(_linear(), wbits=5), F16, "weights must be tile-ordered codes"),
    ("out-bf16", lambda: _set(_linear(), out_dtype=BF16), BF16, "out_dtype must be f32/f16"),
    ("nseg-0", lambda: _set(_linear(), nseg=0), F16, "nseg must be 1 or 2"),
    ("nseg-3", lambda: _set(_linear(), nseg=3), F16, "nseg must be 1 or 2"),
    ("epilogue-int8-geglu", lambda: _set(_linear(), epilogue=1), F16, "linear epilogue only"),
    ("gn-part", lambda: _set(_linear(), gn_part=FAKE), F16, "linear epilogue only"),
    ("upsample", lambda: _set(_linear(), upsample2x=1), F16, "linear epilogue only"),
    ("geglu-two-segments", lambda: _geglu(clens=[32, 32]), F16, "GEGLU epilogue: one segment"),
    ("geglu-cout", lambda: _geglu(Cout=96), F16, "GEGLU epilogue: one segment"),
    ("geglu-out-type", lambda: _set(_geglu(), out_dtype=F32), F16, "out_dtype must be act_dtype"),
    ("geglu-out-type-bf16", lambda: _geglu(act=F16), BF16, "out_dtype must be act_dtype"),
    ("geglu-residual", lambda: _set(_geglu(), residual=FAKE, ldr=128), F16, "takes no residual and no rowbias"),
    ("geglu-rowbias", lambda: _set(_geglu(), rowbias=FAKE, ld_rowbias=128), F16, "takes no residual and no rowbias"),
    ("geglu-ldo-short", lambda: _set(_geglu(), ldo=56), F16, "out rows must be 16-byte aligned"),
    ("geglu-ldo-odd", lambda: _set(_geglu(), ldo=68), F16, "out rows must be 16-byte aligned"),
    ("geglu-out-misaligned", lambda: _set(_geglu(), out=FAKE + 8), F16, "out rows must be 16-byte aligned"),
    ("rowbias-short", lambda: _set(_linear(), rowbias=FAKE, ld_rowbias=39), F16, "ld_rowbias shorter than Cout"),
    ("shape-B", lambda: _set(_linear(), B=0), F16, "bad shape"),
    ("shape-Wo", lambda: _set(_linear(), Wo=0), F16, "bad shape"),
    ("shape-Cout", lambda: _set(_linear(), Cout=0, ldo=0), F16, "bad shape"),
    ("kernel-0", lambda: _set(_linear(), kh=0), F16, "bad kernel/stride"),
    ("stride-0", lambda: _set(_linear(), stride=0), F16, "bad kernel/stride"),
    ("taps-36", lambda: _set(_linear(), kh=6, kw=6), F16, "bad kernel/stride"),
    ("pad-negative", lambda: _set(_linear(), pad_t=-1), F16, "bad padding"),
    ("pad-64", lambda: _set(_linear(), pad_l=64), F16, "bad padding"),
    ("m-overflow", lambda: _set(_linear(), B=32768, H=256, W=256, Ho=256, Wo=256), F16, "M overflows int32"),
    ("ldx-odd", lambda: _set(_linear(), ldx=28), F16, "x/w must be 16-byte aligned"),
    ("x-misaligned", lambda: _set(_linear(), x=FAKE + 8), F16, "x/w must be 16-byte aligned"),
    ("w-misaligned", lambda: _set(_linear(), w=FAKE + 4), F16, "x/w must be 16-byte aligned"),
    ("ldo-short", lambda: _set(_linear(), ldo=39), F16, "ldo / ldr shorter than Cout"),
    ("ldr-short", lambda: _set(_linear(), residual=FAKE, ldr=32), F16, "ldo / ldr shorter than Cout"),
    ("seg0-empty", lambda: _set(_linear(), seg0_clen=0), F16, "segment 0 c0/clen must be multiples of 8"),
    ("seg0-clen-odd", lambda: _set(_linear(), seg0_clen=20), F16, "segment 0 c0/clen must be multiples of 8"),
    ("seg0-c0-odd", lambda: _set(_linear(), seg0_c0=4, ldx=32), F16, "segment 0 c0/clen must be multiples of 8"),
    ("seg0-c0-negative", lambda: _set(_linear(), seg0_c0=-8), F16, "segment 0 c0/clen must be multiples of 8"),
    ("seg1-past-the-row", lambda: _set(_two_seg(), seg1_clen=24), F16, "segment 1 c0/clen must be multiples of 8"),
    ("seg0-no-scale", lambda: _set(_linear(), seg0_scale=None), F16, "segment 0 needs scale (delta_w) and zw"),
    ("seg1-no-zw", lambda: _set(_two_seg(), seg1_zw=None), F16, "segment 1 needs scale (delta_w) and zw"),
    ("seg0-zc", lambda: _set(_linear(), seg0_zc=FAKE), F16, "segment 0: zc / zfill / fill16 must be NULL"),
    ("seg0-zfill", lambda: _set(_linear(), seg0_zfill=FAKE), F16, "segment 0: zc / zfill / fill16 must be NULL"),
    ("seg1-fill16", lambda: _set(_two_seg(), seg1_fill16=FAKE), F16, "segment 1: zc / zfill / fill16 must be NULL"),
    # M = 32767 * 65536 < 2^31 rows in 2^24 - 512 row blocks x 129 column blocks
    ("too-many-tiles", lambda: _set(_linear(), B=32767, H=256, W=256, Ho=256, Wo=256, Cout=16512, ldo=16512), F16, "too many tiles"),
    ("workspace-misaligned", lambda: _lend(_desc(**SD_8x8), AMPLE, FAKE + 8), F16, "splitk_ws must be 16-byte aligned"),
    # two breaches at once: the earlier check of the launcher's order reports
    ("order-pointer-before-res-period", lambda: _set(_linear(), out=None, res_period=4), F16, "null tensor pointer"),
    ("order-res-period-before-wbits", lambda: _set(_linear(), res_period=1, wbits=5), F16, "res_period is not supported"),
    ("order-act-before-out-dtype", lambda: _set(_linear(), out_dtype=BF16), F32, "act_dtype must be QD_F16 or QD_BF16"),
    ("order-nseg-before-epilogue", lambda: _set(_linear(), nseg=3, epilogue=1), F16, "nseg must be 1 or 2"),
    ("order-epilogue-before-geglu", lambda: _set(_geglu(Cout=96), upsample2x=1), F16, "linear epilogue only"),
    ("order-geglu-residual-before-ldo", lambda: _set(_geglu(), residual=FAKE, ldr=128, ldo=68), F16, "takes no residual and no rowbias"),
    ("order-rowbias-before-shape", lambda: _set(_linear(), rowbias=FAKE, ld_rowbias=8, B=0), F16, "ld_rowbias shorter than Cout"),
    ("order-shape-before-ldx", lambda: _set(_linear(), B=0, ldx=28), F16, "bad shape"),
    ("order-padding-before-alignment", lambda: _set(_linear(), pad_t=64, x=FAKE + 2), F16, "bad padding"),
    ("order-ldo-before-segments", lambda: _set(_linear(), ldo=8, seg0_scale=None), F16, "ldo / ldr shorter than Cout"),
    ("order-seg0-before-seg1", lambda: _set(_two_seg(), seg0_zc=FAKE, seg1_clen=4), F16, "segment 0: zc / zfill / fill16 must be NULL"),
    ("order-scale-before-zc", lambda: _set(_linear(), seg0_scale=None, seg0_zc=FAKE), F16, "segment 0 needs scale (delta_w) and zw"),
    ("order-segments-before-workspace", lambda: _set(_lend(_desc(**SD_8x8), AMPLE, FAKE + 8), seg0_zw=None), F16, "segment 0 needs scale"),
]
_IDS = [r[0] for r in REFUSALS]


def test_the_table_starts_from_accepted_descriptors(lib):
    for make in (_linear, _two_seg, _geglu):
        assert _accepted(lib, make())[0] == 1
    assert _accepted(lib, _geglu(act=BF16), BF16) == (1, 0, 2, 0)
    assert _accepted(lib, _lend(_desc(**SD_8x8)))[0] >= 2


@pytest.mark.parametrize("case", REFUSALS, ids=_IDS)
def test_form_refuses(lib, case):
    _, make, act, needle = case
    rc, form, msg = _form(lib, make(), act)
    assert rc != 0 and needle in msg and msg.startswith("qd_conv2d_wq_h16: "), msg
    assert form == (-1, -1, -1, -1)                           # nothing is written for a refused descriptor


@pytest.mark.parametrize("case", REFUSALS, ids=_IDS)
def test_launcher_refuses_with_the_same_message(lib, case):
    """qd_conv2d_wq_h16 itself: refused before any launch (no GPU here), and where the library has the form query, with the
    message the query gave."""
    _, make, act, needle = case
    d = make()
    want = None
    if hasattr(lib, "qd_conv2d_wq_h16_form"):
        rc, _, want = _form(lib, d, act)
        assert rc != 0, "the table holds an accepted descriptor"
    rc = lib.qd_conv2d_wq_h16(ctypes.byref(d) if d is not None else None, act, None)
    msg = lib.qd_last_error().decode()
    assert rc != 0 and needle in msg, msg
    assert want is None or msg == want


def test_form_needs_somewhere_to_write(lib):
    assert lib.qd_conv2d_wq_h16_form(ctypes.byref(_linear()), F16, None) != 0
    assert "null form4" in lib.qd_last_error().decode()


def test_python_wrapper_attaches_the_scratch_as_the_launch_wrapper_does(lib, monkeypatch):
    """hip.conv2d_wq_h16_form: the scratch is lent only to a call that asks for split-K, and the counter does not move."""
    import torch
    from qdiff import engine, hip
    lent = []

    class Scratch:
        def __init__(self, nbytes):
            self.nbytes = nbytes
            lent.append(nbytes)

        def data_ptr(self):
            return FAKE

        def numel(self):
            return self.nbytes

    monkeypatch.setattr(hip, "_ptr", lambda t, name=None: None if t is None else FAKE)
    monkeypatch.setattr(hip, "_splitk_scratch", lambda dev, n: Scratch(n))
    monkeypatch.setattr(engine, "WONLY_SPLITK", [0])
    dd = SD_8x8
    seg = [dict(c0=0, clen=1280, kofs=0, kstep0=0, scale=torch.empty(0), zw=torch.empty(0))]

    def call(splitk):
        return hip.ConvCall(x=torch.empty(0, dtype=torch.float16), w=torch.empty(0, dtype=torch.uint8), out=torch.empty(0), ldx=1280, ldk=0,
                            ldo=1280, B=dd["B"], H=8, W=8, Ho=8, Wo=8, Cout=1280, kh=3, kw=3, stride=1, pad_t=1, pad_l=1, wbits=4,
                            w_tiled=True, segs=seg, splitk=splitk)

    assert hip.conv2d_wq_h16_form(call(None), torch.float16) == (1, 0, 0, 0) and not lent
    sliced = hip.conv2d_wq_h16_form(call(True), torch.float16)
    assert sliced[0] >= 2 and lent == [sliced[0] * _mn4(dd)] and sliced[3] == 1
    assert engine.WONLY_SPLITK == [0]
    with pytest.raises(hip.HipEngineError, match="float16 or bfloat16"):
        hip.conv2d_wq_h16_form(call(True), torch.float32)
