"""The workspace planner behind "workspace_reuse" (include/ymk.h: ymk_op_plan_workspace) on traces, host only.

A trace is what a forward's dry run records: allocation k (call order) has a size and a release position - the number of
allocations made when it was released, -1 = never.  It is alive over positions [k, release) (to the end when never
released).  Every assertion here is a condition a correct plan meets, whatever the planner's heuristics."""
import random

import pytest

from yomitoku_amd import _lib

ALIGN = 256


def _al(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def _until(k, rel, n):
    return n if rel < 0 or rel > n else rel


def _check_plan(sizes, rel):
    n = len(sizes)
    off, peak, live = _lib.plan_workspace(sizes, rel)
    assert len(off) == n
    asz = [_al(s) for s in sizes]
    # alignment, bounds
    for k in range(n):
        assert off[k] % ALIGN == 0 and off[k] >= 0
        assert off[k] + asz[k] <= peak
    # no two allocations alive at the same position share a byte: sweep the positions, keep the live set sorted by offset
    ends = sorted((_until(k, rel[k], n), k) for k in range(n))
    alive, e = set(), 0
    for pos in range(n):
        while e < n and ends[e][0] <= pos:
            alive.discard(ends[e][1])
            e += 1
        lo, hi = off[pos], off[pos] + asz[pos]
        for j in alive:
            assert hi <= off[j] or off[j] + asz[j] <= lo, f"allocations {j} and {pos} overlap in time and in address"
        alive.add(pos)
    # the lower bound, recomputed here
    want_live, cur = 0, 0
    delta = [0] * (n + 1)
    for k in range(n):
        delta[k] += asz[k]
        delta[_until(k, rel[k], n)] -= asz[k]
    for k in range(n):
        cur += delta[k]
        want_live = max(want_live, cur)
    assert live == want_live
    assert live <= peak <= sum(asz)
    # deterministic
    assert _lib.plan_workspace(sizes, rel) == (off, peak, live)
    return off, peak, live


def _random_trace(seed, n):
    rng = random.Random(seed)
    sizes, rel = [], []
    for k in range(n):
        kind = rng.random()
        if kind < 0.5:
            sizes.append(rng.randrange(1, 4096))  # small, unaligned
        elif kind < 0.9:
            sizes.append(ALIGN * rng.randrange(1, 4096))
        else:
            sizes.append(rng.randrange(1 << 20, 1 << 26))
        life = rng.random()
        if life < 0.1:
            rel.append(-1)  # never released
        elif life < 0.7:
            rel.append(k + 1 + rng.randrange(0, 6))  # a temporary (may point past the end: lives to the end)
        else:
            rel.append(k + 1 + rng.randrange(0, n))
    return sizes, rel


@pytest.mark.parametrize("seed,n", [(1, 3000), (2, 2500), (3, 4000), (4, 17), (5, 1)])
def test_random_traces(seed, n):
    sizes, rel = _random_trace(seed, n)
    _check_plan(sizes, rel)


def test_empty_trace():
    assert _lib.plan_workspace([], []) == ([], 0, 0)


def test_chain_needs_only_its_largest_buffer():
    # each buffer is released before the next is taken: nothing is ever alive together
    sizes = [ALIGN * v for v in (3, 9, 1, 7, 9, 2, 40, 5)]
    rel = [k + 1 for k in range(len(sizes))]
    off, peak, live = _check_plan(sizes, rel)
    assert peak == max(sizes) == live
    assert off == [0] * len(sizes)
    # unaligned sizes: the largest, rounded up
    sizes = [1000, 5, 70000, 300]
    _, peak, _ = _check_plan(sizes, [1, 2, 3, 4])
    assert peak == _al(70000)


def test_producer_consumer_chain_needs_two_buffers():
    # x_k is read by the launch that writes x_{k+1}: released after the next allocation
    sizes = [ALIGN * 10] * 12
    rel = [k + 2 for k in range(12)]
    _, peak, live = _check_plan(sizes, rel)
    assert peak == live == 2 * ALIGN * 10


def test_nothing_released_is_the_bump_arena():
    sizes = [ALIGN * v for v in (5, 1, 8, 8, 2, 100, 3)]
    _, peak, live = _check_plan(sizes, [-1] * len(sizes))
    assert peak == sum(sizes) == live
    sizes = [1, 257, 1000, 4096, 77]
    _, peak, _ = _check_plan(sizes, [-1] * len(sizes))
    assert peak == sum(_al(s) for s in sizes)
    # a release position at or past the end means the same
    _, peak, _ = _check_plan(sizes, [len(sizes)] * len(sizes))
    assert peak == sum(_al(s) for s in sizes)


def test_all_dead_at_once():
    # everything is taken first and released together, then one more buffer: it fits where the others were
    sizes = [ALIGN * v for v in (4, 6, 2, 8)] + [ALIGN * 15]
    rel = [4, 4, 4, 4, -1]
    off, peak, live = _check_plan(sizes, rel)
    assert live == ALIGN * 20 == peak
    assert off[4] == 0


def test_resnet_block_pattern():
    """x -> t1 (1x1) -> t2 (3x3) -> [sh (shortcut)] -> y = 1x1(t2) + sh; t1 dies once t2 is written, t2 / sh / x once y is.
    Sixteen blocks at one resolution: a bump arena takes the sum, the plan stays at the live bound."""
    c, s = ALIGN * 64, ALIGN * 256
    sizes, rel = [s], [None]  # x of the first block
    x = 0
    for blk in range(16):
        short = blk % 4 == 0
        t1 = len(sizes); sizes.append(c); rel.append(None)
        t2 = len(sizes); sizes.append(c); rel.append(None)
        rel[t1] = len(sizes)  # released right after t2's launch
        if short:
            sh = len(sizes); sizes.append(s); rel.append(None)
        y = len(sizes); sizes.append(s); rel.append(None)
        rel[t2] = len(sizes)
        if short:
            rel[sh] = len(sizes)
        rel[x] = len(sizes)
        x = y
    rel[x] = -1
    _, peak, live = _check_plan(sizes, rel)
    assert live == 3 * s + c  # x, sh, y and t2 at the end of a block with a shortcut
    assert peak == live
    assert peak < sum(sizes) // 4


def test_long_lived_buffers_do_not_fragment_the_plan():
    # a PARSeq-like trace: buffers that span the forward, a large early phase, a smaller late phase taking its bytes
    keep = [ALIGN * 3, ALIGN * 50, ALIGN]
    early = [ALIGN * v for v in (100, 100, 300, 100, 400)]
    late = [ALIGN * v for v in (20, 20, 40, 20, 80, 5, 5)]
    sizes = keep + early + late
    n_keep, n_early = len(keep), len(early)
    rel = [-1] * n_keep + [n_keep + n_early] * n_early + [-1] * len(late)
    _, peak, live = _check_plan(sizes, rel)
    assert live == sum(keep) + sum(early)
    assert peak == live


def test_bad_traces_are_refused():
    with pytest.raises(_lib.YmkError):
        _lib.plan_workspace([256, 256], [-1, 1])  # released before it was made
    with pytest.raises(_lib.YmkError):
        _lib.plan_workspace([256, 256], [0, -1])
    with pytest.raises(_lib.YmkError):
        _lib.plan_workspace([-5], [-1])


def test_switches_exist_without_a_device():
    lib = _lib.load()
    for key in ("workspace_reuse", "workspace_poison"):
        assert lib.ymk_debug_option(key.encode(), 0) == 0, key
    for key in ("workspace_planned_forwards", "ws_plan_bytes_last", "ws_bump_bytes_last", "ws_live_bound_last"):
        assert _lib.stat(key) >= 0
