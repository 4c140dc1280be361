"""Host checks of the exact-row attention cases (tests/attn_exact_cases.py): every condition the GPU test relies on, and the
evidence that the new criterion sees what the statistical one (<= 1 % of outputs beyond 2e-4 * range, none beyond 2e-2 * range)
lets through — eight mistakes planted in a copy of the oracle, each on the case built for it."""
import numpy as np
import pytest
import torch

import attn_exact_cases as A
from oracle import quant_ref as R


@pytest.fixture(scope="module")
def cases():
    return A.all_cases()


def _heads(t, B, L, H, d):
    return t.view(B, L, H, d).permute(0, 2, 1, 3).reshape(B * H, L, d)


def test_conditions_hold_for_every_case(cases):
    """>= 90 % of the rows decided and every feature row decided; 'dense long' states its mean undecided keys per row."""
    assert len(cases) >= 60
    for c in cases.values():
        if c.stated_undecided:
            mean = float(c.ev.undecided_per_row.mean())
            print(f"{c.name}: mean undecided keys per row {mean:.1f} of {c.S}")
            assert 0 < mean < c.S
            continue
        assert c.decided.mean() >= 0.9, (c.name, float(c.decided.mean()))
        assert c.features and all(c.decided[bh, i] for bh, i in c.features), c.name


def test_operand_codes_survive_the_quantiser(cases):
    for c in cases.values():
        for x, codes, aq, L, pre in ((c.q, c.qc, c.aq_q, c.T, c.prescale), (c.k, c.kc, c.aq_k, c.S, c.prescale), (c.v, c.vc, c.aq_v, c.S, 1.0)):
            got = R.uaq_codes(_heads(x, c.B, L, c.H, c.d) * pre, aq["delta"], aq["zero_point"], aq["n_bits"], aq["sym"])
            assert np.array_equal(got.numpy(), codes), c.name


def test_builder_matches_the_integer_oracle_on_decided_rows(cases):
    for c in cases.values():
        want, _ = R.attention_int(_heads(c.q, c.B, c.T, c.H, c.d), _heads(c.k, c.B, c.S, c.H, c.d), _heads(c.v, c.B, c.S, c.H, c.d),
                                  c.scale, c.aq_q, c.aq_k, c.aq_v, c.aq_w, pre_scale=c.prescale)
        mine = c.I.astype(np.float64) * (float(c.aq_w["delta"]) * float(c.aq_v["delta"]))
        dec = c.decided
        assert np.array_equal(want.numpy()[dec], mine[dec]), c.name


def test_edge_classes_are_reached(cases):
    """The values each class exists for, computed from the oracle's integers."""
    assert np.abs(cases["epi_dw2^-24_S160_clamped"].I).max() == 160 * 65535 * 255 > 2 ** 31
    assert 2 ** 30 < np.abs(cases["epi_dw2^-23_S256"].I).max() < 2 ** 31
    assert cases["epi_dw2^-22_S128_small"].ev.pu.sum(-1).max() == 2 ** 22
    b = cases["bytes_p16"]
    tops = {int(b.ev.pu[0, i].max()) for i in range(b.T)}
    assert {255, 256, 257, 32767, 32768, 65535} <= tops
    assert (b.ev.c[0].max(-1) > 65536 - 1e-3).any()                      # above the grid: the clamped body
    hi_live = b.ev.pu.max(-1) >= 256
    assert hi_live[:, :128].sum(-1).tolist() == [1, 1] and not hi_live[:, 128:256].any()
    d = cases["dynamics_S77"]
    assert (d.ev.s[:, 0].argmax(-1) == d.S - 1).all()                    # maximum in the last key of the ragged tail
    cs2 = d.spec.cs * A.LOG2E
    assert ((d.ev.s.max(-1) - d.ev.s[:, :, :32].max(-1)) * cs2 > 64).any()  # rises > 64 octaves after tile 0
    assert (d.ev.s[:, 8].max(-1) == d.ev.s[:, 8].min(-1)).all()          # equal scores
    assert ((d.ev.s.max(-1, keepdims=True) - d.ev.s) * cs2 > 126).any()  # exp2 underflows
    for name in ("sat_d256_zq0_zk0_zv0", "sat_d80_zq0_zk0_zv0"):
        s = cases[name]
        ks = ((s.qc - s.spec.zq)[:, :, None, :] * (s.kc[:, None, :, :] - 128)).sum(-1)      # the kernel's own sum_d q~ k'
        assert np.abs(ks).max() >= s.d * 255 * 127 and np.abs(ks).max() < (2 ** 22 if s.d < 128 else 2 ** 23)
        assert s.ev.pu[:, 0].max() == 65535 and (np.abs(s.vc - s.spec.zv) == 255).any()


def test_margin_is_positive_and_grows_with_the_code():
    c = np.linspace(0.0, 70000.0, 2001)
    for S, L, rise, ubias in ((1, 0.0, 0.0, 0.0), (77, 5.0, 90.0, 128.0), (4096, 0.3, 0.0, 0.0)):
        m = A.margin(c, L, 1.0, rise, 4 * A.U, S, 0.003, ubias)
        assert (m > 0).all() and (np.diff(m) > 0).all()
        assert m[0] < 1e-4 and m[-1] < 0.5 + 70000 * 1e-4


# ---- planted mistakes -----------------------------------------------------------------------------------------------------
def _oracle(c, mistake=None):
    """The oracle of attn_exact_cases.evaluate, restated with one planted mistake; float32 rows [BH, T, d]."""
    sp = c.spec
    s = A._exact_matmul(c.qc - sp.zq, np.swapaxes(c.kc - sp.zk, 1, 2))
    vt = c.vc - sp.zv
    S, T = c.S, c.T
    tail0 = (S // 32) * 32 if S % 32 else S - 32
    if mistake == "drop_last_key":
        s, vt = s[:, :, :-1], vt[:, :-1]
    if mistake == "miss_max_of_last_tile":                                  # the last tile's scores never raise the maximum
        s = s.copy()
        s[:, :, tail0:] = np.minimum(s[:, :, tail0:], s[:, :, :tail0].max(-1, keepdims=True))
    pu, _, _, _ = A.softmax_codes(s, sp.cs, sp.dw, sp.zpw, sp.wmin, sp.wmax)
    if mistake == "shift_ragged_tile_keys":
        vt = vt.copy()
        vt[:, tail0:S - 1] = vt[:, tail0 + 1:S].copy()
    if mistake == "wrap_hi_byte_at_256":
        pu = pu % 256
    if mistake == "wrap_hi_byte_at_32768":
        pu = np.where(pu >= 32768, pu - 65536, pu)
    I = A._exact_matmul(pu, vt)
    if mistake == "wrap_I_to_32_bits":
        I = ((I + 2 ** 31) % 2 ** 32) - 2 ** 31
    out = (I.astype(np.float32) * np.float32(np.float32(sp.dw) * np.float32(sp.dv))).astype(np.float32)
    if mistake == "swap_two_heads":
        out = out.copy()
        out[[0, 1]] = out[[1, 0]]
    if mistake == "row_T-1_from_the_wrong_wave":
        out = out.copy()
        out[:, T - 1] = out[:, T - 1 - 32]
    return out


PLANTED = [("drop_last_key", "geom_S77_T129_d40"), ("shift_ragged_tile_keys", "geom_S77_T129_d40"),
           ("wrap_hi_byte_at_256", "bytes_p16"), ("wrap_hi_byte_at_32768", "bytes_p16"),
           ("wrap_I_to_32_bits", "epi_dw2^-24_S160_clamped"), ("miss_max_of_last_tile", "dynamics_S77"),
           ("swap_two_heads", "geom_S65_T129_d40"), ("row_T-1_from_the_wrong_wave", "geom_S77_T129_d40")]


def test_planted_mistakes_are_caught(cases):
    """Each mistake fails the decided-row criterion on its case; the table says whether the statistical criterion of
    test_attention_fused would have passed the same data."""
    lines = []
    for mistake, name in PLANTED:
        c = cases[name]
        ok0, _ = A.check_rows(c, _oracle(c))
        assert ok0, (name, "the unmodified oracle must pass")
        got = _oracle(c, mistake)
        ok, rep = A.check_rows(c, got)
        want_int = c.I.astype(np.float64) * (c.spec.dw * c.spec.dv)
        old = A.old_criterion(got, want_int)
        lines.append(f"{mistake:30s} {name:28s} new: {'passes' if ok else 'FAILS '} ({rep.bad_decided} outputs)   old 1 % / 2e-2: {'passes' if old else 'fails'}")
        assert not ok, (mistake, name)
    print("\nplanted mistake                case                         criterion")
    print("\n".join(lines))
