"""CPU tests of the helpers behind test_bench_batch_parity_gpu.py (tests/bench_batch_cases.py): the replica order, the replica
comparator, and the case list against the batches bench.py states."""
import math

import pytest
import torch

import bench_batch_cases as BB
from golden_util import fixture_inputs, load_fixture


@pytest.mark.parametrize("n", [2, 8, 10, 16, 64])
def test_thue_morse_order_balances_the_sources(n):
    order = BB.thue_morse(n)
    assert order[:8] == [0, 1, 1, 0, 1, 0, 0, 1][:min(n, 8)]
    assert order == [bin(i).count("1") % 2 for i in range(n)]
    assert order.count(0) == order.count(1) == n // 2                      # even n: whole aligned pairs, one of each source
    if n >= 8:
        for src in (0, 1):
            where = [i for i, s in enumerate(order) if s == src]
            # both halves of a 128-row tile at a 64-row level, every quarter of a 256-row tile
            assert {i % 2 for i in where} == {0, 1}
            assert {i % 4 for i in where} == {0, 1, 2, 3}
        for p in range(0, n - 1, 2):                                       # every aligned pair holds both sources
            assert {order[p], order[p + 1]} == {0, 1}


def test_plain_alternation_would_not():
    """What the order is for: 0 1 0 1 ... keeps a source on one parity."""
    alt = [i % 2 for i in range(16)]
    assert {i % 2 for i, s in enumerate(alt) if s == 0} == {0}


def test_replicate_follows_the_order():
    x = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4)
    t = torch.tensor([5, 9])
    xn, tn, cn = BB.replicate((x, t, None), 10)
    assert cn is None and xn.shape == (10, 3, 4) and xn.is_contiguous()
    assert tn.tolist() == [5, 9, 9, 5, 9, 5, 5, 9, 9, 5]
    assert all(torch.equal(xn[i], x[s]) for i, s in enumerate(BB.thue_morse(10)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_comparator_flags_one_ulp_in_one_element(dtype):
    g = torch.Generator().manual_seed(3)
    src = torch.randn(2, 4, 8, 8, generator=g).to(dtype)
    y = src[torch.tensor(BB.thue_morse(16))].clone()
    assert BB.replica_mismatch(y) is None
    pos, el = 11, (2, 5, 3)
    v = y[pos][el].clone()
    y[pos][el] = torch.nextafter(v, torch.tensor(math.inf, dtype=dtype))   # one ulp up
    assert y[pos][el] != v
    msg = BB.replica_mismatch(y)
    assert msg is not None and msg.startswith(f"position {pos} (source {BB.thue_morse(16)[pos]}) differs from position ")
    assert "on 1 of 256 elements" in msg and "1 of 16 positions differ" in msg
    assert f"{float((y[pos][el].double() - v.double()).abs()):.3e}" in msg
    y[pos][el] = v
    assert BB.replica_mismatch(y) is None


def test_comparator_is_bitwise():
    """+0 against -0 is a difference (torch.equal would let it pass); a NaN in the same place of every replica is none."""
    y = torch.zeros(4, 3)
    y[2, 1] = -0.0
    assert torch.equal(y[2], y[1]) and BB.replica_mismatch(y) is not None and BB.replica_mismatch(y).startswith("position 2 ")
    y = torch.ones(4, 3)
    y[:, 0] = float("nan")
    assert BB.replica_mismatch(y) is None
    y[3, 0] = 1.0                                                           # position 3 holds source 0, like position 0
    msg = BB.replica_mismatch(y)
    assert msg.startswith("position 3 (source 0) differs from position 0") and "inf" in msg


def test_comparator_names_the_first_of_several_and_the_first_replica_is_the_reference():
    y = torch.arange(2.0)[torch.tensor(BB.thue_morse(8))].view(8, 1).repeat(1, 5)
    y[5, 0] += 1.0
    y[6, 4] += 0.5
    msg = BB.replica_mismatch(y)
    assert msg.startswith("position 5 (source 0) differs from position 0") and "2 of 8 positions differ" in msg and "1.000e+00" in msg
    y2 = y.clone()
    y2[0, 1] += 2.0                               # the reference replica itself: every other replica of source 0 now differs
    msg = BB.replica_mismatch(y2)
    assert msg.startswith("position 3 (source 0) differs from position 0") and "3 of 8 positions differ" in msg and "2.000e+00" in msg


def test_form_counts():
    counts = BB.form_counts([(128, 160, 256, 1), None, (256, 160, 256, 1), (128, 160, 256, 1)])
    assert counts == [((128, 160, 256, 1), 2), ((256, 160, 256, 1), 1)]
    assert BB.forms_line(counts) == "128x160/256t/k1 x2, 256x160/256t/k1 x1"


def test_cases_are_the_benchmarks_batches():
    """The evaluation batches bench.py measures, as literals (bench.py is a yardstick: it is read, never imported).
      bench.py:590   --images-per-gpu defaults to 8; a CFG evaluation holds 2n samples (bench.py:3, :811)      -> sd 16
      bench.py:685-686  --full adds --extra-batch 5 = evaluation batch 10 next to the headline                   -> sd 10
      bench.py:513   extra_lines runs ("cifar", 64) and ("ldm", 64); both unguided (guide 1.0: batch n, :811)  -> cifar 64, ldm 64
      bench.py:514-516  the ldm child also gets --extra-batch 10 (README.md:47-49 `-n 10`)                      -> ldm 10
    """
    sd_images, sd_extra_images, cfg_factor = 8, 5, 2
    line_batches = {"cifar": 64, "ldm": 64}
    ldm_extra = 10
    want = {("sd_full", cfg_factor * sd_images), ("sd_full", cfg_factor * sd_extra_images), ("ldm_full", ldm_extra),
            ("ldm_full", line_batches["ldm"]), ("cifar_full", line_batches["cifar"])}
    assert set(BB.CASES) == want and len(BB.CASES) == len(want)
    assert set(BB.PAIR_CASES) == {("sd_full", sd_images), ("sd_full", sd_extra_images), ("sd_tiny", sd_images)}
    assert all(n % 2 == 0 for _, n in BB.CASES)                            # balanced sources in every case


def test_ldm_full_at_64_passes_the_row_bound_of_the_embedding_kernel():
    """hip.temb_mlp launches in row groups once B * K floats pass its LDS bound (44 KiB of fp32 words: 44 * 1024 // K rows per
    launch).  The residual blocks' embedding Linears read the time embedding, K = 4 * model_channels: 896 for LDM-4, so batch 64
    takes two launches (50 + 14 rows) and batch 10 one; SD (K = 1280) fits its 16 rows in one."""
    K = 4 * load_fixture("model_ldm_full.pt")["spec"]["unet"]["model_channels"]
    assert K == 896 and (44 * 1024) // K == 50
    assert [n for name, n in BB.CASES if name == "ldm_full" and n > 50] == [64]
    K_sd = 4 * load_fixture("model_sd_full.pt")["spec"]["unet"]["model_channels"]
    assert (44 * 1024) // K_sd >= 16


@pytest.mark.parametrize("name,n", BB.PAIR_CASES)
def test_pair_inputs_are_distinct(name, n):
    fx = load_fixture(f"model_{name}.pt")
    xh, th, ctx = BB.pair_inputs(fixture_inputs(fx, "test"), n, "cpu")
    assert xh.shape[0] == th.shape[0] == n and ctx.shape[0] == 2 * n
    assert len(set(th.tolist())) == n
    for a in (xh, ctx):
        flat = a.flatten(1)
        assert all(not torch.equal(flat[i], flat[j]) for i in range(len(flat)) for j in range(i))
    x, t, c = fixture_inputs(fx, "test")
    assert torch.equal(xh[:2], x) and torch.equal(th[:2], t) and torch.equal(ctx[:2], c)
