"""tests/quantized_counter_ref.py, the numpy restatement of lsp::dspu::QuantizedCounter, against what the reference's own class
recorded into tests/golden/quantized_counter_ref_vectors.npz: the counters and every state word after every operation and the ring
after the last, bit for bit.  No GPU.

Also here: the closed form of one call (what the kernel runs) against the reference's counted loop over a sweep of heads, counts,
periods, capacities and call lengths; the invariant that the counters sum to nCount; the reference's long-call defect, pinned by one
recorded case; and five deliberate errors that the recorded cases must each catch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import quantized_counter_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_quantized_counter_vectors as gen  # noqa: E402

f32, u32 = np.float32, np.uint32
X, CASES = gen.load()
PLAIN = [c for c in CASES if not c["name"].startswith(gen.DEFECT)]


def ids(cases):
    return [c["name"].replace(" ", "_") for c in cases]


def replay(c, closed_form=False, mutation=None):
    """The words after every operation and the ring after the last, as the restatement has them."""
    q = Q.QuantizedCounter(c["max_period"], c["max_levels"], mutation=mutation)
    words = []
    for op in c["ops"]:
        Q.apply(q, op, X, closed_form)
        words.append(q.settings_words())
    return np.stack(words), q.history.view(u32).copy(), q


def test_the_stored_file_is_the_generators_case_list():
    want = gen.cases()
    assert [c["name"] for c in CASES] == [c["name"] for c in want]
    assert np.array_equal(X.view(u32), gen.rows().view(u32))
    for a, b in zip(CASES, want):
        assert a["max_period"] == b["max_period"] and a["max_levels"] == b["max_levels"] and np.array_equal(a["ops"], b["ops"]), a["name"]
    assert os.path.getsize(gen.OUT) < 400 * 1000


def test_the_cases_cover_what_they_must():
    codes = {int(op[0]) for c in CASES for op in c["ops"]}
    assert codes == set(range(10))
    assert np.array_equal(X[gen.ROW_SPECIAL, :14].view(u32), np.array(gen.SPECIALS, f32).view(u32))
    # the 14 specials: what the compiled reference gave
    first = CASES[0]["words"][-1]
    assert CASES[0]["name"].startswith(gen.X86) and list(first[:8]) == [2, 0, 0, 0, 1, 0, 0, 1] and first[16] == 9 and first[17] == 1
    # every call size at every offset of the row's base from the 16-byte grid
    sizes = {(int(c["ops"][-1][3]), int(c["ops"][-1][2]) % 4) for c in CASES if c["name"].startswith("call of")}
    assert sizes >= {(n, b) for n in (0, 1, 3, 255, 256, 257, 1023, 1024, 1025, 4096) for b in range(4)}
    # calls beyond nCapacity - nPeriod (outside the reference's exact domain), beyond nCapacity, and between nPeriod and nCapacity
    beyond = over = between = at_end = 0
    for c in PLAIN:
        cap = Q.capacity_of(c["max_period"])
        for k, op in enumerate(c["ops"]):
            if int(op[0]) == Q.PROCESS:
                n, period, head = int(op[3]), int(c["words"][k][-6]), int(c["words"][k][-8])
                beyond += n > cap - period
                over += n > cap
                between += period < n < cap
                at_end += head == 0 and n > 0
    assert beyond >= 10 and over >= 3 and between >= 10 and at_end >= 1
    # count() above period() after a set_period, a pending update at a process and at an update_settings, a clear
    above = sum(int(w[-7]) > int(w[-6]) for c in PLAIN for w in c["words"])
    assert above >= 5
    # a subnormal range; an empty one (the step is Inf); a reversed one (the step is negative)
    steps = np.array([w[-2] for c in PLAIN for w in c["words"]], u32).view(f32)
    assert np.isinf(steps).any() and (steps < 0).any() and (steps > 1e38).any()
    assert ((X[gen.ROW_SUBNORMAL] != 0) & (np.abs(X[gen.ROW_SUBNORMAL]) < 1.17e-38)).sum() > 100
    assert {c["max_levels"] for c in CASES} == {16, 300}


@pytest.mark.parametrize("index", range(len(CASES)), ids=ids(CASES))
def test_restatement_is_the_reference_in_every_bit(index):
    c = CASES[index]
    words, ring, _ = replay(c)
    bad = np.argwhere(words != c["words"])
    assert bad.size == 0, (c["name"], "operation %d, word %d" % tuple(bad[0]), c["ops"][bad[0][0]])
    assert np.array_equal(ring, c["ring"]), c["name"]


@pytest.mark.parametrize("index", range(len(PLAIN)), ids=ids(PLAIN))
def test_closed_form_is_the_reference_in_every_bit(index):
    """process() as the kernel forms it: one plan per call, the final window counted directly."""
    c = PLAIN[index]
    words, ring, _ = replay(c, closed_form=True)
    assert np.array_equal(words, c["words"]) and np.array_equal(ring, c["ring"]), c["name"]


def test_counters_sum_to_the_count_after_every_operation():
    for c in PLAIN:
        ml = c["max_levels"]
        for k, w in enumerate(c["words"]):
            assert int(w[:ml + 2].astype(np.int64).sum()) == int(w[ml + 3]), (c["name"], k)
            assert w[-1] or not w[int(w[ml + 5]):ml].any(), (c["name"], k, "a counter beyond nLevels")


def test_closed_form_against_the_counted_loop():
    """make_plan() against the reference's loop fed in pieces, over heads, counts, periods, capacities and call lengths: the samples
    are their own serial numbers, so the window, the ring and every eviction are checked by identity."""
    rng = np.random.default_rng(5)
    checked = 0
    for max_period in (1, 5, 40, 100):
        cap = Q.capacity_of(max_period)
        for period in sorted({1, max_period, (max_period + 1) // 2}):
            for head in (0, 1, cap // 2, cap - 2, cap - 1):
                for count in sorted({0, 1, period - 1, period, min(cap, period + 3), min(cap, max_period + 7), cap} - {-1}):
                    for n in (0, 1, 3, period - 1, period, period + 1, cap - period - 1, cap - period, cap - period + 1, cap - 1, cap, cap + 1,
                              2 * cap + 5, int(rng.integers(1, 3 * cap))):
                        if n < 0:
                            continue
                        q = Q.QuantizedCounter(max_period, 4)
                        q.set_range(0.0, 4.0, 4)
                        q.set_period(period)
                        q.update_settings()
                        q.history[:] = (1000000 + np.arange(cap)).astype(f32)          # every word of the ring is its own
                        q.head, q.count = head, count
                        data = np.arange(n, dtype=f32) + f32(0.5)
                        pl = Q.make_plan(head, count, period, cap, n)
                        old = q._span(pl["tail"], count)
                        q.process(data)
                        # the window afterwards: the newest count_after of (what was held, then the row)
                        seen = np.concatenate([old, data])
                        assert q.count == pl["count_after"] == min(min(count, period) + n, period) and q.head == pl["head_after"]
                        assert np.array_equal(q._span((q.head + cap - q.count) % cap, q.count), seen[len(seen) - q.count:])
                        assert pl["evict"] + pl["remain"] == count and pl["remain"] + (n - pl["keep_from"]) == q.count
                        assert np.array_equal(np.concatenate([old[pl["evict"]:], data[pl["keep_from"]:]]), seen[len(seen) - q.count:])
                        # the ring: the plan's stores on the old words
                        ring = (1000000 + np.arange(cap)).astype(f32)
                        stored = data[pl["store_from"]:]
                        ring[(pl["store_pos"] + np.arange(len(stored))) % cap] = stored
                        assert len(stored) <= cap and np.array_equal(ring, q.history)
                        checked += 1
    assert checked > 2000


def test_the_references_single_long_call_is_a_defect_that_is_pinned():
    """One call of 4096 samples on a ring of 2032 with a period of 900: the reference's loop overwrites samples that are not evicted
    yet and takes the wrong ones out.  The restatement with its defect flag gives the recorded words; the sliding window does not,
    though sum, head and count agree."""
    c = next(c for c in CASES if c["name"].startswith(gen.DEFECT))
    pieces = next(c for c in CASES if c["name"] == "the same row in pieces")
    assert np.array_equal(c["ops"][:2], pieces["ops"][:2]) and list(c["ops"][2][1:]) == list(pieces["ops"][2][1:])
    assert int(c["ops"][2][0]) == Q.PROCESS_WHOLE and int(c["ops"][2][3]) == 4096 > Q.capacity_of(1000) - 900
    words, ring, _ = replay(c)
    assert np.array_equal(words, c["words"]) and np.array_equal(ring, c["ring"])
    a, b = c["words"][-1], pieces["words"][-1]
    assert not np.array_equal(a[:18], b[:18]) and a[:18].sum() == b[:18].sum() == 900 and np.array_equal(a[18:], b[18:])
    assert np.array_equal(c["ring"], pieces["ring"])
    # the sliding window IS the histogram of the last 900 samples
    want = np.bincount(Q.bin_words(X[gen.ROW_UNIFORM, 4096 - 900:4096], f32(-1.3), Q.rstep_of(16, -1.3, 1.3), 16, 16), minlength=18)
    assert np.array_equal(b[:18], want)
    # inside the domain a single call is exact: 1100 <= 2032 - 900
    for n in (700, 1100):
        one, cut = Q.QuantizedCounter(1000, 16, defect=True), Q.QuantizedCounter(1000, 16)
        for q in (one, cut):
            q.set_range(-1.3, 1.3, 16)
            q.set_period(900)
            q.process(X[gen.ROW_UNIFORM, :900])
        one.process(X[gen.ROW_SINE, :n])
        for at in range(0, n, 512):
            cut.process(X[gen.ROW_SINE, at:min(n, at + 512)])
        assert np.array_equal(one.state_words(), cut.state_words()), n


@pytest.mark.parametrize("mutation", Q.MUTATIONS)
def test_a_deliberate_error_is_caught_by_a_recorded_case(mutation):
    caught = []
    for c in PLAIN:
        words, ring, _ = replay(c, mutation=mutation)
        if not np.array_equal(words, c["words"]):
            caught.append(c["name"])
    assert caught, mutation
    if mutation in ("nan_bin0", "inf_above"):
        assert all(n.startswith(gen.X86) for n in caught), caught          # the group that is named for it, and no other


def test_the_bin_rule_on_the_specials():
    words = Q.bin_words(np.array(gen.SPECIALS, f32), f32(-1.0), Q.rstep_of(8, -1.0, 1.0), 8, 16)
    #            NaN +Inf -Inf 1e30 -1e30 -1.05 -1.2 -1.25 -1.26 1.0 0.999999 -0.0 7.5e8 5.4e8
    assert list(words) == [16, 16, 16, 16, 16, 0, 0, 16, 16, 17, 7, 4, 16, 16]
    # 5.4e8 + 1 scales to just above 2^31: below; 5.3e8 scales to less: above
    assert list(Q.bin_words(np.array([5.3e8], f32), f32(-1.0), f32(4.0), 8, 16)) == [17]


def test_the_shared_header_on_the_host_is_the_restatement(tmp_path):
    """csrc/quantized_counter_bank.h compiled for the host (tests/cpp/quantized_counter_plan.cpp): bin_of() over every recorded row
    under six ranges and four level counts, and make_plan() over a sweep that ends at calls of 2^31 - 1 samples."""
    exe, src, dst = str(tmp_path / "plan"), str(tmp_path / "x.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "lsp-dsp-units_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "quantized_counter_plan.cpp"), "-o", exe])
    x = X.reshape(-1)
    x.tofile(src)
    subprocess.check_call([exe, src, dst])
    raw, at = np.fromfile(dst, u32), 0
    for lo, hi in ((-1, 1), (-0.5, 0.25), (0.0, 2.4e-38), (1, -1), (0.3, 0.3), (-1e30, 1e30)):
        for levels in (1, 8, 16, 300):
            rstep = Q.rstep_of(levels, lo, hi)
            assert raw[at] == rstep.view(u32), (lo, hi, levels)
            got, at = raw[at + 1:at + 1 + len(x)], at + 1 + len(x)
            assert np.array_equal(got, Q.bin_words(x, f32(lo), rstep, levels, 300)), (lo, hi, levels)
    plans = raw[at:].reshape(-1, 13)
    assert len(plans) > 2000 and plans[:, 4].max() == 2 ** 31 - 1
    for w in plans:
        cap, period, head, count, n = (int(v) for v in w[:5])
        p = Q.make_plan(head, count, period, cap, n)
        assert [int(v) for v in w[5:]] == [p[k] for k in ("tail", "evict", "remain", "keep_from", "store_from", "store_pos", "head_after", "count_after")], w[:5]
