"""Cases and helpers of test_bench_batch_parity_gpu.py / test_bench_batch_parity_host.py: whole quantised UNets at the
evaluation batches bench.py measures ("measured batches").

TEST INFRASTRUCTURE.  Every whole-model golden holds two samples (golden_util.fixture_inputs), and the batch decides the launch
forms: four-wave blocks, the 256-row tile, the split-K slice counts, grouped q / k / v members of 128 rows, GroupNorm
statistics from the epilogue instead of the partial pass behind split-K, the row groups of hip.temb_mlp.  The cases below keep
the fixture's two samples and scale NOTHING but the batch: the samples are replicated to N, so that

  * every replica must equal the first replica of its source bit for bit (samples are independent in the reference,
    qdiff/quant_block.py:190-221; the library has no float atomics and its per-sample statistics chunk by S only), and
  * positions 0 and 1 are still the two samples the reference golden and the fp64 oracle were computed for.

The order of the replicas is the Thue-Morse sequence (source = parity of popcount(i): 0 1 1 0 1 0 0 1 ...).  Plain alternation
would put a source on the same half of every 128-row tile at a 64-row level and on the same quarter of every 256-row tile.
"""
import torch

# (fixture, evaluation batch): bench.py's batches, see test_bench_batch_parity_host.py::test_cases_are_the_benchmarks_batches
CASES = [("sd_full", 16), ("sd_full", 10), ("ldm_full", 10), ("ldm_full", 64), ("cifar_full", 64)]
# (fixture, guidance pairs n): evaluation batch 2n with equal halves
PAIR_CASES = [("sd_full", 8), ("sd_full", 5), ("sd_tiny", 8)]


def case_id(c):
    return f"{c[0]}-b{c[1]}"


def thue_morse(n):
    """Source index (0 / 1) of each of n positions."""
    return [bin(i).count("1") & 1 for i in range(n)]


def replicate(inputs, n):
    """The fixture's (x, t, context-or-None) of two samples replicated to n in Thue-Morse order."""
    idx = torch.tensor(thue_morse(n))
    return tuple(None if a is None else a[idx].contiguous() for a in inputs)


def replica_mismatch(y, order=None):
    """None when every y[i] is bit-equal to y[first position of its source]; otherwise a message that names the first position
    that differs, how many positions do, and the largest |difference|.  Compares bit patterns: a NaN equals itself, +0 != -0."""
    order = thue_morse(y.shape[0]) if order is None else list(order)
    assert len(order) == y.shape[0]
    first = {}
    for i, s in enumerate(order):
        first.setdefault(s, i)
    bits = y.contiguous().view(torch.int32 if y.element_size() == 4 else torch.int16 if y.element_size() == 2 else torch.int64)
    bad = [i for i, s in enumerate(order) if not torch.equal(bits[i], bits[first[s]])]
    if not bad:
        return None
    i = bad[0]
    j = first[order[i]]
    n_el = int((bits[i] != bits[j]).sum())
    worst = max(float((y[k].double() - y[first[order[k]]].double()).abs().nan_to_num(nan=float("inf")).max()) for k in bad)
    return (f"position {i} (source {order[i]}) differs from position {j} on {n_el} of {y[i].numel()} elements; "
            f"{len(bad)} of {len(order)} positions differ, max |diff| = {worst:.3e}")


def form_counts(forms):
    """Multiset of (rows, columns, threads, K slices) of the launches `launch_forms` saw, as a sorted list of (form, count)."""
    out = {}
    for f in forms:
        if f is not None:
            out[tuple(f)] = out.get(tuple(f), 0) + 1
    return sorted(out.items())


def forms_line(counts):
    return ", ".join(f"{r}x{c}/{t}t/k{k} x{n}" for (r, c, t, k), n in counts)


def pair_inputs(fx_inputs, n, device, seed=77):
    """n guidance pairs from a fixture with a context: xh = the fixture's two latents + seeded draws, distinct timesteps,
    2n distinct context rows.  Returns (xh, th, context) on `device`."""
    x, t, c = fx_inputs
    g = torch.Generator().manual_seed(seed)
    xh = torch.cat([x, torch.randn((n - 2,) + tuple(x.shape[1:]), generator=g)])
    th = torch.cat([t, (t[0] + 53 * torch.arange(1, n - 1)) % 1000]).to(t.dtype)
    assert len(set(th.tolist())) == n, "timesteps of the pairs must be distinct"
    ctx = torch.cat([c, torch.randn((2 * n - 2,) + tuple(c.shape[1:]), generator=g)])
    return xh.to(device), th.to(device), ctx.to(device)
