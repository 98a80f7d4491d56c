"""Reads tests/golden/filter_ref_designs.npz and filter_ref_streams.npz (written by tests/golden/make_filter_vectors.py from the
reference's own compiled Filter and FilterBank classes) and replays the stream cases on the oracle's recurrence.  Never reads the
reference tree; oracle/_ref/ only through the tests that say so.

A design: sample_rate, fp (nType, nSlope, fFreq, fFreq2, fGain, fQuality as given), sections float32 [k, 5] as FilterBank::chain(i)
returned them after update() + rebuild(), inactive, latency, limited (get_params() after Filter::limit), chart (APO designs only, else
None: freq_chart() at chart_frequencies(sample_rate), complex64 [16]).

A stream case: name, shared (0: the filter owns its bank; 1 / 2: a bank shared with a second filter `other` whose sections go ahead
of / behind this filter's; 3: a shared bank with this filter alone, which is an Equalizer of one filter), sample_rate, fp, other,
calls, events [(ahead of which call, kind, a, fp)] with kind 0 update(a = sample rate, fp), 1 impulse_response(a samples), 2
clear(); x; and what the reference did: sections (per call, float32 [k, 5], of the whole bank in its order), inactive, latency and
limited per call, out, irs (one row per impulse_response event)."""
import io
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DESIGNS = os.path.join(GOLDEN, "filter_ref_designs.npz")
STREAMS = os.path.join(GOLDEN, "filter_ref_streams.npz")
MAGIC = 0x464c5452
UPDATE, IMPULSE, CLEAR, CHART = range(4)
FLT_NONE = 0
FILTER_CHAINS_MAX = 0x80


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def canon(a):
    """float32 with every NaN made the one canonical quiet NaN: which sign and payload a 0 / 0 of the designer leaves (a frequency
    limited to 0) differs between two builds of the same text and means nothing."""
    a = np.array(a, f32, copy=True)
    a[np.isnan(a)] = np.nan
    return a


def fp_words(fp):
    """filter_params_t as six 32-bit words."""
    return np.concatenate([np.array(fp[:2], np.uint32), bits(np.array(fp[2:], f32))])


def fp_tuple(words):
    w = np.ascontiguousarray(words, np.uint32)
    f = w[2:].view(f32)
    return (int(w[0]), int(w[1]), f[0], f[1], f[2], f[3])


def chart_frequencies(sample_rate):
    """The 16 frequencies of a recorded chart: 20 Hz to 0.6 of the sample rate, so that the last ones are past the clamp at half of
    it (Filter.cpp:576).  Plain float32 products, the same on every machine."""
    step = f32((0.6 * sample_rate / 20.0) ** (1.0 / 15.0))
    out = [f32(20.0)]
    for _ in range(15):
        out.append(f32(out[-1] * step))
    return np.array(out, f32)


def design_case(sample_rate, fp, chart=False):
    """A design as a case of the driver: one call of no samples, which only rebuilds; chart: freq_chart() ahead of it."""
    events = [(0, CHART, 16, (0, 1, 0.0, 0.0, 1.0, 0.0), chart_frequencies(sample_rate))] if chart else []
    return dict(name="design", shared=0, sample_rate=int(sample_rate), fp=fp, other=(0, 1, 0.0, 0.0, 1.0, 0.0), calls=[0], events=events,
                x=np.zeros(0, f32))


def case_bytes(cases):
    """The case file of oracle/filter_driver.cpp (its head comment has the layout)."""
    b = io.BytesIO()
    u32 = lambda *v: b.write(np.array(v, np.uint32).tobytes())
    u32(MAGIC, len(cases))
    for c in cases:
        u32(c["shared"], c["sample_rate"])
        b.write(fp_words(c["fp"]).tobytes())
        b.write(fp_words(c["other"]).tobytes())
        u32(len(c["calls"]), *c["calls"])
        u32(len(c["events"]))
        for e in c["events"]:
            u32(*e[:3])
            b.write(fp_words(e[3]).tobytes())
            if e[1] == CHART:
                assert len(e[4]) == e[2]
                b.write(np.ascontiguousarray(e[4], f32).tobytes())
        assert len(c["x"]) == sum(c["calls"])
        u32(len(c["x"]))
        b.write(np.ascontiguousarray(c["x"], f32).tobytes())
    return b.getvalue()


def parse_results(raw, cases):
    """What a driver wrote: per case a dict of sections, inactive, latency, limited (lists per call), out and irs."""
    w = np.frombuffer(raw, np.uint32)
    pos, out = 0, []

    def take(n):
        nonlocal pos
        v = w[pos:pos + n]
        assert len(v) == n, "short result file"
        pos += n
        return v

    for c in cases:
        ncalls = int(take(1)[0])
        assert ncalls == len(c["calls"])
        r = dict(sections=[], inactive=[], latency=[], limited=[])
        for _ in range(ncalls):
            k = int(take(1)[0])
            r["sections"].append(canon(take(5 * k).view(f32).reshape(k, 5)))
            r["inactive"].append(int(take(1)[0]))
            r["latency"].append(int(take(1)[0]))
            r["limited"].append(take(6).copy())
        r["out"] = canon(take(int(take(1)[0])).view(f32))
        assert len(r["out"]) == len(c["x"])
        r["irs"] = [take(int(take(1)[0])).view(f32).copy() for _ in range(int(take(1)[0]))]
        assert len(r["irs"]) == sum(1 for e in c["events"] if e[1] == IMPULSE)
        r["charts"] = []
        for _ in range(int(take(1)[0])):
            m = int(take(1)[0])
            v = take(4 * m).view(f32).copy()
            r["charts"].append(dict(packed=v[0:2 * m:2] + 1j * v[1:2 * m:2], split=v[2 * m:3 * m] + 1j * v[3 * m:]))
        assert len(r["charts"]) == sum(1 for e in c["events"] if e[1] == CHART)
        out.append(r)
    assert pos == len(w), "result file longer than its cases"
    return out


def load_designs(path=DESIGNS):
    z = np.load(path)
    ends = np.cumsum(z["nsec"])
    charts = dict(zip((int(i) for i in z["chart_of"]), z["chart"]))
    out = []
    for i in range(len(z["nsec"])):
        out.append(dict(sample_rate=int(z["sample_rate"][i]), fp=fp_tuple(z["fp"][i]), sections=z["sections"][ends[i] - z["nsec"][i]:ends[i]],
                        inactive=int(z["inactive"][i]), latency=int(z["latency"][i]), limited=z["limited"][i], chart=charts.get(i)))
    return out


def load_streams(path=STREAMS):
    z = np.load(path)
    cases = []
    pc = pe = ps = po = pi = pr = 0
    for i, name in enumerate(z["names"]):
        n, nc, ne = int(z["n"][i]), int(z["ncalls"][i]), int(z["nevents"][i])
        c = dict(name=str(name), shared=int(z["shared"][i]), sample_rate=int(z["sample_rate"][i]), fp=fp_tuple(z["fp"][i]),
                 other=fp_tuple(z["other"][i]), calls=[int(v) for v in z["calls"][pc:pc + nc]],
                 events=[(int(e[0]), int(e[1]), int(e[2]), fp_tuple(e[3:])) for e in z["events"][pe:pe + ne]],
                 x=z["x"][int(z["at"][i]):int(z["at"][i]) + n], out=z["out"][po:po + n],
                 inactive=[int(v) for v in z["inactive"][pc:pc + nc]], latency=[int(v) for v in z["latency"][pc:pc + nc]],
                 limited=[w for w in z["limited"][pc:pc + nc]], sections=[], irs=[])
        for k in z["nsec"][pc:pc + nc]:
            c["sections"].append(z["sections"][ps:ps + int(k)])
            ps += int(k)
        for _ in range(sum(1 for e in c["events"] if e[1] == IMPULSE)):
            m = int(z["ir_len"][pr])
            c["irs"].append(z["ir"][pi:pi + m])
            pi, pr = pi + m, pr + 1
        pc, pe, po = pc + nc, pe + ne, po + n
        cases.append(c)
    return cases


def limit(sample_rate, fp):
    """Filter::limit (Filter.cpp:161-167) -> the limited (nType, nSlope, fFreq, fFreq2, fGain, fQuality)."""
    top = f32(0.49) * f32(sample_rate)
    lim = lambda v: min(max(f32(v), f32(0.0)), top)
    return (int(fp[0]), min(max(int(fp[1]), 1), FILTER_CHAINS_MAX), lim(fp[2]), lim(fp[3]), f32(fp[4]), f32(fp[5]))


def boundaries(case):
    """What every call of the case starts with, from the reference's own text: Filter::update sets FF_CLEAR where the limited type or
    slope differs from the one before (Filter.cpp:154-158), clear() sets it, init() sets it; rebuild() hands it to FilterBank::end
    only where the filter owns its bank (:399-400), and end() clears the delays where it is told to or where the number of sections
    differs from the one before the last begin() (FilterBank.cpp:233).  -> per call (rebuilt, cleared); an impulse_response event
    rebuilds as well, ahead of the call it stands ahead of."""
    own = case["shared"] == 0
    cur, clear = limit(case["sample_rate"], case["fp"]), True
    pending, last = True, None
    out = []
    for i in range(len(case["calls"])):
        rebuilt = cleared = False
        count = len(case["sections"][i])

        def settle():
            nonlocal pending, clear, last, rebuilt, cleared
            if pending:
                rebuilt = True
                cleared = cleared or (own and clear) or count != last
                pending, clear, last = False, False, count

        for before, kind, a, fp in case["events"]:
            if before != i:
                continue
            if kind == UPDATE:
                new = limit(a, fp)
                clear = clear or new[0] != cur[0] or new[1] != cur[1]
                cur, pending = new, True
            elif kind == CLEAR:
                clear, pending = True, True
            else:
                settle()
        settle()
        out.append((rebuilt, cleared))
    return out


def replay(case, oracle, cleared=None, sections=None):
    """The oracle's static recurrence (oracle.biquad_cascade) through the case's calls on the recorded sections (or the given ones),
    the delays cleared where boundaries() says (or where `cleared`, a list per call, says) -> (out, irs)."""
    cleared = [b[1] for b in boundaries(case)] if cleared is None else cleared
    sections = case["sections"] if sections is None else sections
    out, irs = np.zeros(len(case["x"]), f32), []
    state, pos = None, 0
    for i, n in enumerate(case["calls"]):
        sec = sections[i]
        if cleared[i] or state is None or len(state) != max(len(sec), 1):
            state = np.zeros((max(len(sec), 1), 2), f32)
        for before, kind, a, _ in case["events"]:
            if before == i and kind == IMPULSE:
                irs.append(oracle.biquad_impulse_response(a, sec, state.copy()))
        out[pos:pos + n], state = oracle.biquad_cascade(case["x"][pos:pos + n], sec, state)
        pos += n
    return out, irs


def replay_f64(case, oracle, cleared=None):
    """The same in float64 on the recorded float32 sections: the round-off yardstick."""
    cleared = [b[1] for b in boundaries(case)] if cleared is None else cleared
    out = np.zeros(len(case["x"]), np.float64)
    state, pos = None, 0
    for i, n in enumerate(case["calls"]):
        sec = case["sections"][i]
        if cleared[i] or state is None or len(state) != len(sec):
            state = np.zeros((len(sec), 2))
        out[pos:pos + n], state = oracle.biquad_cascade_f64_state(case["x"][pos:pos + n], sec, state)
        pos += n
    return out
