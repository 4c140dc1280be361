"""The kernel-choice rule of the fused int8 attention (csrc/attn_i8.hip: attn_policy, plan()), on a machine without a GPU.
qd_attn_i8_form is the launcher itself with the launch withheld — a pure host function, so it runs here on fake 16-byte aligned
pointers — and abi_emulator.attn_i8_form is the rule written down from the table of DESIGN.md 4.4.  They agree over a sweep across
every break point of the rule under every knob state; qd_attn_uses_keyterm and qd_attn_ws_bytes are corollaries of the same rule;
the query refuses what the launcher refuses, in the launcher's words; and the exact-row suite reaches every instantiation the
launcher can name.  Whoever changes the policy changes its statement too, and the GPU tests that assert their kernel by the query
keep meaning what they say."""
import ctypes
import itertools

import pytest

import abi_emulator

FAKE = 0x1000                                   # never followed: the query makes no HIP call and reads no operand
DIMS = sorted(set(range(8, 257, 8)) | {20, 60, 100})
KEYS = (1, 77, 511, 512, 4096, 16384, 16385)
KNOBS = list(itertools.product((0, 2, 3), (0, 1), (0, 1, 3)))          # (pipe, ktab, lean)
BUILT_DT = {1, 2, 3, 4, 5, 8}                   # attn_kernel's head-dim pads; every lean dim has DT <= 3
# THE set of instantiations (family, DT, term mode or ASYM, probability bits)
INSTANCES = ({(0, dt, a, w) for dt in (1, 2, 3, 4, 5, 8) for a in (0, 1) for w in (8, 16)}
             | {(1, dt, kt, w) for dt in (1, 2, 3) for kt in (0, 1, 2) for w in (8, 16)}
             | {(2, dt, kt, w) for dt in (1, 2) for kt in (0, 2) for w in (8, 16)})


def pad32(n):
    return (n + 31) // 32 * 32


@pytest.fixture
def attn_lib():
    from qdiff import hip
    lib = hip.load()
    try:
        yield lib
    finally:
        lib.qd_attn_config(2, -1, 1, 1)


def _args(d, S, q_asym, have_kterm, wbits=16, BH=2, H=1, T=129, **over):
    a = dict(q=FAKE, k=FAKE, vt=FAKE, qsum=None, kterm=FAKE if have_kterm else None, vsum=FAKE, BH=BH, H=H, T=T, S=S, d=d,
             Tpad=pad32(T), Spad=pad32(S), dpad=pad32(d), prm=FAKE, wbits=wbits, wmin=0, wmax=(1 << wbits) - 1, q_asym=1 if q_asym else 0,
             out=FAKE, ldo=H * d, out8=None, ldo8=0, oq_params=None, oq_min=0, oq_max=0, oq_off=0, ws=FAKE, ws_bytes=1 << 40,
             last=None, q_heads=BH)
    a.update(over)
    return a


def query(lib, **a):
    """form4 of the call, or the launcher's refusal as a string."""
    form = (ctypes.c_int32 * 4)()
    a = dict(a, last=form if a["last"] is None else a["last"])
    if lib.qd_attn_i8_form(*a.values()):
        return lib.qd_last_error().decode()
    return tuple(form)


def test_keyterm_and_workspace_queries_are_corollaries_of_the_rule(attn_lib):
    """qd_attn_uses_keyterm = "with a table passed, the term mode is 2"; qd_attn_ws_bytes != 0 = "with a table, or with a symmetric
    q, the family is 2", and then 16 bytes per padded query + 4 per 128-query block.  Both entries are older than the rule's one
    function: this test passes unchanged on the library of the commit before it, which is the evidence that the rule did not move."""
    lib = attn_lib
    BH, T = 2, 129
    for pipe, ktab, lean in KNOBS:
        lib.qd_attn_config(pipe, -1, ktab, lean)
        E = lambda *a: abi_emulator.attn_i8_form(*a, pipe=pipe, ktab=ktab, lean=lean)
        for d, S in itertools.product(DIMS, KEYS):
            for asym in (0, 1):
                assert lib.qd_attn_uses_keyterm(d, S, asym) == int(E(d, S, asym, True)[2] == 2), (pipe, ktab, lean, d, S, asym)
            ws = lib.qd_attn_ws_bytes(BH, T, S, d)
            assert (ws != 0) == (E(d, S, 1, True)[0] == 2 or E(d, S, 0, False)[0] == 2), (pipe, ktab, lean, d, S)
            assert ws in (0, BH * pad32(T) * 16 + BH * ((T + 127) // 128) * 4)


def test_attention_form_query_states_the_rule(attn_lib):
    lib = attn_lib
    seen = set()
    for pipe, ktab, lean in KNOBS:
        lib.qd_attn_config(pipe, -1, ktab, lean)
        for d, S, asym, have, wbits in itertools.product(DIMS, KEYS, (0, 1), (False, True), (8, 16)):
            got = query(lib, **_args(d, S, asym, have, wbits))
            want = abi_emulator.attn_i8_form(d, S, asym, have, pipe=pipe, ktab=ktab, lean=lean)
            where = (pipe, ktab, lean, d, S, asym, have, wbits)
            if want[0] == 0 and want[1] not in BUILT_DT:
                assert got == f"qd_attn_i8: head dim pad {pad32(d)} unsupported (32,64,96,128,160,256)", where
                continue
            assert got == want, where
            assert got[3] == (3 if got[0] == 2 else 1)
            seen.add(got[:3] + (wbits,))
            if have:
                assert lib.qd_attn_uses_keyterm(d, S, asym) == int(got[2] == 2), where
    assert seen == INSTANCES, sorted(seen ^ INSTANCES)


REFUSALS = [
    ("null operand", dict(vsum=None), "qd_attn_i8: null pointer"),
    ("wbits 12", dict(wbits=12), "qd_attn_i8: probability bits must be 8 or 16 (got 12)"),
    ("grid wider than its bits", dict(wbits=8, wmin=0, wmax=256), "qd_attn_i8: probability grid [0,256] wider than 8 bits"),
    ("Tpad", dict(Tpad=136), "qd_attn_i8: padded dims must be multiples of 32"),
    ("q_heads", dict(BH=6, H=2, q_heads=4), "qd_attn_i8_qp: q_heads (4) must divide BH (6) and be a multiple of H (2)"),
    ("ldo", dict(ldo=1 << 24), "qd_attn_i8: output row stride must be below 2^24 elements (got 16777216)"),
    ("dpad 192", dict(d=192, dpad=192, ldo=192), "qd_attn_i8: head dim pad 192 unsupported (32,64,96,128,160,256)"),
    ("dpad 224", dict(d=200, dpad=224, ldo=200), "qd_attn_i8: head dim pad 224 unsupported (32,64,96,128,160,256)"),
]


@pytest.mark.parametrize("over,text", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_attention_form_query_refuses_what_the_launcher_refuses(attn_lib, over, text):
    lib = attn_lib
    a = dict(_args(40, 77, 1, False), **over)
    assert query(lib, **a) == text
    # ... and the launcher says the same: the refusal comes from the plan, before anything is launched (asked only now that the
    # query has refused, so that nothing can reach the device)
    assert lib.qd_attn_i8_qp(*dict(a, last=None).values()) != 0
    assert lib.qd_last_error().decode() == text


def test_attention_form_query_needs_its_own_output(attn_lib):
    lib = attn_lib
    assert lib.qd_attn_i8_form(*dict(_args(40, 77, 1, False), last=None).values()) != 0
    assert lib.qd_last_error().decode() == "qd_attn_i8_form: null form4"


def test_attention_workspace_is_checked_on_the_lds_staged_plan_only(attn_lib):
    lib = attn_lib
    BH, T, S, d = 2, 129, 4096, 40
    need = lib.qd_attn_ws_bytes(BH, T, S, d)
    assert need == BH * 160 * 16 + BH * 2 * 4
    assert query(lib, **_args(d, S, 1, True, ws_bytes=need)) == (2, 2, 2, 3)
    short = query(lib, **_args(d, S, 1, True, ws_bytes=need - 1))
    assert short == f"qd_attn_i8: this shape needs {need} bytes of 16-byte aligned workspace (qd_attn_ws_bytes), got {need - 1}"
    assert query(lib, **_args(d, S, 1, True, ws=None, ws_bytes=0)).startswith(f"qd_attn_i8: this shape needs {need} bytes")
    # no table for an asymmetric q: the register-fed kernel, which takes no workspace (qd_attn_ws_bytes is an upper bound)
    assert query(lib, **_args(d, S, 1, False, ws=None, ws_bytes=0)) == (1, 2, 1, 1)
    assert query(lib, **_args(d, 77, 1, True, ws=None, ws_bytes=0)) == (1, 2, 1, 1)


def test_exact_row_suite_reaches_every_instantiation(attn_lib):
    """The union of the forms of the form_d* cases of tests/attn_exact_cases.py under every knob triple forms_of() returns for them,
    with the table hip.attn_i8 would build, is the launcher's whole list."""
    import attn_exact_cases as A
    from test_attention_exact_gpu import forms_of
    lib = attn_lib
    seen = set()
    for name, c in A.all_cases().items():
        if not name.startswith("form_d"):
            continue
        asym = not c.spec.qsym
        for label, pipe, ktab, lean, want in forms_of(c.d, asym):
            lib.qd_attn_config(pipe, -1, ktab, lean)
            have = bool(lib.qd_attn_uses_keyterm(c.d, c.S, asym))
            got = query(lib, **_args(c.d, c.S, asym, have, c.spec.wbits, BH=c.B * c.H, H=c.H, T=c.T))
            assert got == want, (name, label)
            seen.add(got[:3] + (c.spec.wbits,))
    assert seen == INSTANCES, sorted(seen ^ INSTANCES)
