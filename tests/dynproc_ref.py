"""CPU yardsticks for lsp::dspu::DynamicProcessor (src/main/dynamics/DynamicProcessor.cpp) for the tests, in the manner of
compressor_ref.py.

follow_literal()  the loop of process() (:404-430) with solve_reaction (:195-202), sample by sample and channel by channel, as
                  the reference writes it: numpy float32 scalars, every product and sum rounded once.
follow()          the same vectorised across channels over tables padded with a level of +inf; a host test holds the two
                  against each other bit for bit.  Also counts how often each branch and each table entry was taken.
gain64()          reduction() / curve() / model() in float64 on float32 inputs and float32 spline parameters; lx = ln x is
                  the float32 value on both sides, and the branches of every spline are chosen on it.
gain32()          the same in float32, logf / expf taken as the correctly rounded values.
gain_bound()      the a-priori relative bound on |float32 gain - gain64| in units of u = 2^-24, see below.
params64()        update_settings() (:339-395) with sort_reactions, sort_splines and hermite_quadratic in float64 with the
                  running first-order bound of compressor_ref.Q (u per operation, 4 u per logf / expf, carried through the
                  quotients dy / dx and (k0 - k1) / (x0 - x1)).

The gain bound, per sample, with lx = logf(x) carrying LIBM u |lx| (LIBM = 4 u for logf and for expf), per spline j:
    line:   t = lx - thresh, p = ratio t, a = makeup + p
                                            Dt = LIBM u |lx| + u |t|,  D_j = |ratio| Dt + u |p| + u |a|
    knee:   q = h0 lx + h1, r = q lx, a = r + h2        (as compressor_ref has it)
                                            Dq = |h0 lx| (LIBM + 1) u + |q| u
                                            D_j = |lx| Dq + |q lx| (LIBM + 1) u + |a| u
    sum:    gain_j = gain_(j-1) + a_j       one rounding per partial sum: u |gain_j|
    bound = (sum_j D_j + sum_j |gain_j| + LIBM) SLACK, + 1 for curve() and model() (the product with x)
No spline: gain = expf(+0) = 1 exactly, bound 0.
"""
import numpy as np

from compressor_ref import LIBM, SLACK, U, Q, hold_samples  # noqa: F401

f32 = np.float32
DOTS, RANGES = 4, 5
GAIN_AMP_MIN, FLOAT_SAT_M_INF, FLOAT_SAT_P_INF = f32(1e-6), f32(1e-10), f32(1e10)
BRANCHES = ("attack", "release", "hold", "rearm")


def fresh_state(C):
    return {"e": np.zeros(C, f32), "peak": np.zeros(C, f32), "hold": np.zeros(C, np.uint32)}


# ---- the follower -------------------------------------------------------------------------------------------------------
def solve_reaction(table, x):
    """:195-202, table: list of {"level", "tau"}; returns (tau, index of the entry taken)"""
    r, k = f32(table[0]["tau"]), 0
    for i in range(1, len(table)):
        if x >= f32(table[i]["level"]):
            r, k = f32(table[i]["tau"]), i
    return r, k


def follow_literal(x, state, params):
    """x: float32 [C, n]; state as fresh_state(), advanced in place; params: per-channel dicts (get_params).  The envelope."""
    x = np.ascontiguousarray(x, f32)
    C, n = x.shape
    env = np.empty((C, n), f32)
    for c in range(C):
        e, peak, hold = f32(state["e"][c]), f32(state["peak"][c]), int(state["hold"][c])
        p = params[c]
        for i in range(n):
            s = x[c, i]
            d = f32(s - e)
            if d < 0:
                if hold > 0:
                    hold -= 1
                else:
                    e = f32(e + f32(d * solve_reaction(p["release"], e)[0]))
                    peak = e
            else:
                e = f32(e + f32(d * solve_reaction(p["attack"], e)[0]))
                if e >= peak:
                    peak = e
                    hold = int(p["hold"])
            env[c, i] = e
        state["e"][c], state["peak"][c], state["hold"][c] = e, peak, hold
    return env


def _tables(params, name):
    C = len(params)
    lvl, tau = np.full((C, RANGES), np.inf, f32), np.zeros((C, RANGES), f32)
    for c, p in enumerate(params):
        for i, r in enumerate(p[name]):
            lvl[c, i], tau[c, i] = r["level"], r["tau"]
    lvl[:, 0] = -np.inf                                         # entry 0 is the default whatever its level says
    return lvl, tau


def _solve(lvl, tau, x):
    idx = np.zeros(x.shape, np.int64)
    for i in range(1, RANGES):
        idx = np.where(x >= lvl[:, i], i, idx)
    return tau[np.arange(len(x)), idx], idx


def follow(x, state, params, lookup_after_step=False):
    """As follow_literal(), across channels at once.  Returns (envelope, taken): taken counts the BRANCHES and, per table, how
    often each entry was selected on a sample that used it ("attack_entry" / "release_entry": int [C, 5]).
    lookup_after_step is a deliberate MISREADING (tau looked up from e + tau0 d) that a host test shows to give other bits."""
    x = np.ascontiguousarray(x, f32)
    C, n = x.shape
    al, at = _tables(params, "attack")
    rl, rt = _tables(params, "release")
    nhold = np.array([p["hold"] for p in params], np.uint32)
    e, peak, hold = state["e"].astype(f32), state["peak"].astype(f32), state["hold"].astype(np.uint32)
    env = np.empty((C, n), f32)
    taken = dict.fromkeys(BRANCHES, 0)
    taken["attack_entry"], taken["release_entry"] = np.zeros((C, RANGES), np.int64), np.zeros((C, RANGES), np.int64)
    one, rows = np.uint32(1), np.arange(C)
    for i in range(n):
        d = x[:, i] - e
        neg = d < 0
        held = neg & (hold > 0)
        src = e
        if lookup_after_step:
            src = e + np.where(neg, _solve(rl, rt, e)[0], _solve(al, at, e)[0]) * d
        (ta, ia), (tr, ir) = _solve(al, at, src), _solve(rl, rt, src)
        en = e + d * np.where(neg, tr, ta)                      # float32 arrays: the product rounds, then the sum
        rearm = ~neg & (en >= peak)
        rel = neg & ~held
        np.add.at(taken["attack_entry"], (rows[~neg], ia[~neg]), 1)
        np.add.at(taken["release_entry"], (rows[rel], ir[rel]), 1)
        taken["attack"] += int(np.count_nonzero(~neg))
        taken["release"] += int(np.count_nonzero(rel))
        taken["hold"] += int(np.count_nonzero(held))
        taken["rearm"] += int(np.count_nonzero(rearm))
        e = np.where(held, e, en)
        peak = np.where(rel | rearm, en, peak)
        hold = np.where(held, hold - one, np.where(rearm, nhold, hold)).astype(np.uint32)
        env[:, i] = e
    state["e"], state["peak"], state["hold"] = e, peak, hold
    return env, taken


# ---- the curve ----------------------------------------------------------------------------------------------------------
def limited(e, lo):
    """|e| limited to [lo, FLOAT_SAT_P_INF], float32"""
    return np.clip(np.abs(np.ascontiguousarray(e, f32)), f32(lo), FLOAT_SAT_P_INF).astype(f32)


def _curve(e, params, dtype, lo, model, shift=0):
    """(gain, bound in u, which) of the level e [C, n] in `dtype` arithmetic.  which: int8 [C, n, 4], per spline 0 below
    knee_start (model: at or below thresh), 1 inside the knee, 2 from knee_stop on (model: above thresh), -1 no such spline.
    shift: the branches are chosen on lx moved by that many float32 spacings (the arithmetic stays on lx): the branch a logf
    takes that is `shift` ulp from the correctly rounded one, see gain_bound_either()."""
    x32 = limited(e, lo)
    C, n = x32.shape
    lx32 = np.log(x32.astype(np.float64)).astype(f32)          # logf, correctly rounded: the float32 value both sides use
    lx = lx32.astype(dtype)
    for _ in range(abs(shift)):                                 # from here on lx32 only chooses branches
        lx32 = np.nextafter(lx32, f32(np.inf if shift > 0 else -np.inf))
    gain, D = np.zeros((C, n), dtype), np.zeros((C, n))
    which = np.full((C, n, DOTS), -1, np.int8)
    count = np.array([len(p["splines"]) for p in params])
    for j in range(DOTS):
        on = (count > j)[:, None]
        col = lambda name, k=None: np.array([(p["splines"][j][name] if k is None else p["splines"][j][name][k])
                                             if len(p["splines"]) > j else 0.0 for p in params], f32)[:, None]
        ks, ke, th, mk, pre, post = (col(nm) for nm in ("knee_start", "knee_stop", "thresh", "makeup", "pre_ratio", "post_ratio"))
        h0, h1, h2 = (col("herm", k).astype(dtype) for k in range(3))
        if model:
            below, above = lx32 <= th, lx32 > th
        else:
            below = lx32 <= ks
            above = ~below & (lx32 >= ke)
        ratio = np.where(below, pre, post).astype(dtype)
        t = lx - th.astype(dtype)
        p = ratio * t
        al = mk.astype(dtype) + p
        q = h0 * lx + h1
        r = q * lx
        ah = r + h2
        line = below | above
        a = np.where(line, al, ah)
        dl = np.abs(ratio) * (LIBM * np.abs(lx) + np.abs(t)) + np.abs(p) + np.abs(al)
        dq = np.abs(h0 * lx) * (LIBM + 1) + np.abs(q)
        dh = np.abs(lx) * dq + np.abs(r) * (LIBM + 1) + np.abs(ah)
        new = gain + np.where(on, a, dtype(0.0))
        D += np.where(on, np.where(line, dl, dh).astype(np.float64) + np.abs(new.astype(np.float64)), 0.0)
        gain = new.astype(dtype)
        which[:, :, j] = np.where(on, np.where(below, 0, np.where(above, 2, 1)), -1)
    g = np.exp(gain.astype(np.float64)).astype(dtype)
    bound = np.where((count > 0)[:, None], (D + LIBM) * SLACK, 0.0)
    return g, bound, which


def gain64(e, params, lo=GAIN_AMP_MIN, model=False):
    return _curve(e, params, np.float64, lo, model)[0]


def gain32(e, params, lo=GAIN_AMP_MIN, model=False):
    return _curve(e, params, f32, lo, model)[0]


def gain_bound(e, params, lo=GAIN_AMP_MIN, model=False):
    """Allowed |gain - gain64| / gain64 in units of u = 2^-24, per sample (0 for a channel without splines: the gain is 1)."""
    return _curve(e, params, np.float64, lo, model)[1]


def gain_bound_either(e, params, lo=GAIN_AMP_MIN, model=False):
    """gain_bound() for an implementation whose logf is not the correctly rounded one.  The splines choose their branch on
    lx = logf(x); LIBM allows logf 2 ulp, so at a level whose logarithm lies within 2 ulp of a knee end or a threshold either
    branch is a correct evaluation.  The two meet there in value and slope, but their bounds differ (the knee's monomial
    form cancels, the line's does not): allowed is, over the branch choices of lx - 2 ulp .. lx + 2 ulp, the largest of that
    choice's own bound plus the distance of its float64 value from gain64()'s, in u."""
    g0, b0, _ = _curve(e, params, np.float64, lo, model)
    out = b0
    with np.errstate(all="ignore"):
        for shift in (-2, -1, 1, 2):
            g, b, _ = _curve(e, params, np.float64, lo, model, shift)
            out = np.maximum(out, b + np.where(g == g0, 0.0, np.abs(g - g0) / g0 / U))
    return out


def within(got, g64, bound):
    """got (float32 results) against g64 under the relative bound (in u), sample by sample; returns (ok, err in u).  The bound is
    derived for an expf that neither underflows nor overflows: where g64 is below the smallest normal float32 the result is a
    subnormal or 0 (absolute spacing 2^-149: the relative bound at 2^-126 plus one spacing), above the largest it is that or inf."""
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    tiny, huge = 2.0 ** -126, float(np.finfo(f32).max)
    with np.errstate(all="ignore"):
        err = np.abs(got - g64) / g64 / U
        ok = np.where(g64 < tiny, np.abs(got - g64) <= bound * U * tiny + 2.0 ** -149,
                      np.where(g64 > huge, got >= huge * (1.0 - bound * U), err <= bound))
    return ok, np.where((g64 < tiny) | (g64 > huge), 0.0, err)


def branches(e, params, lo=GAIN_AMP_MIN, model=False):
    return _curve(e, params, np.float64, lo, model)[2]


# ---- update_settings() in float64 with a first-order error bound -------------------------------------------------------
def _sorted(pairs):
    """The exchange sort of sort_reactions / sort_splines on the first field (stable enough: the order among equals is the
    reference's, which a test with equal levels would need)."""
    s = [list(p) for p in pairs]
    for i in range(len(s) - 1):
        for j in range(i + 1, len(s)):
            if s[j][0] < s[i][0]:
                s[i], s[j] = s[j], s[i]
    return s


def params64(sample_rate=0, hold=0.0, in_ratio=1.0, out_ratio=1.0, dots=(), attack_levels=(), release_levels=(),
             attack_times=(0.0,), release_times=(0.0,)):
    """Every quantity of update_settings() as a Q, keyed like flatten(); the inputs are the float32 values the setters keep."""
    sr = float(f32(sample_rate))
    k707 = Q(float(f32(1.0 - np.sqrt(0.5)))).log()
    ms = Q(float(f32(0.001)))
    out = {}
    with np.errstate(all="ignore"):
        for name, levels, times in (("attack", attack_levels, attack_times), ("release", release_levels, release_times)):
            times = [float(f32(t)) for t in times] + [0.0] * (RANGES - len(times))
            tab = [(0.0, times[0])]
            for i, lv in enumerate(levels):
                if lv is not None and lv >= 0:
                    tab.append((float(f32(lv)), times[i + 1]))
            for i, (lv, t) in enumerate(_sorted(tab)):
                out["%s%d.level" % (name, i)] = Q(lv)
                # a time of 0: k707 / 0 = -inf, expf(-inf) = 0, tau = 1 exactly
                out["%s%d.tau" % (name, i)] = Q(1.0) if t * sr == 0.0 else 1.0 - (k707 / (Q(t) * ms * sr)).exp()
        s = _sorted([[float(f32(v)) for v in d] for d in dots if d is not None and min(d) >= 0])
        sub = Q(0.0)
        for i, (inp, outp, knee) in enumerate(s):
            pre = Q(float(f32(in_ratio))) - 1.0 if i == 0 else Q(0.0)
            if i + 1 < len(s):
                dx = (Q(s[i + 1][0]) / inp).log()
                dy = (Q(s[i + 1][1]) / outp).log()
                post = dy / dx - 1.0
            else:
                post = 1.0 / Q(float(f32(out_ratio))) - 1.0
            post = post - sub if i > 0 else post                # 0 is subtracted exactly from the first
            sub = sub + post if i > 0 else post
            thresh, lk = Q(inp).log(), Q(knee).log()
            stop, start = thresh - lk, thresh + lk
            makeup = Q(outp).log() - thresh if i == 0 else Q(0.0)
            y1 = makeup + pre * lk if i == 0 else Q(0.0)        # makeup = pre = 0 from the second spline on: exact
            p0 = (pre - post) * 0.5 / (start - stop)
            p1 = pre - Q(2.0) * p0 * start
            p2 = y1 - (p0 * start + p1) * start
            for nm, v in (("pre_ratio", pre), ("post_ratio", post), ("knee_start", start), ("knee_stop", stop), ("thresh", thresh),
                          ("makeup", makeup), ("herm0", p0), ("herm1", p1), ("herm2", p2)):
                out["spline%d.%s" % (i, nm)] = v
    return out


def flatten(p):
    """A get_params / compute_params dict with the keys of params64()."""
    out = {}
    for name in ("attack", "release"):
        for i, r in enumerate(p[name]):
            out["%s%d.level" % (name, i)] = float(r["level"])
            out["%s%d.tau" % (name, i)] = float(r["tau"])
    for i, s in enumerate(p["splines"]):
        for nm in ("pre_ratio", "post_ratio", "knee_start", "knee_stop", "thresh", "makeup"):
            out["spline%d.%s" % (i, nm)] = float(s[nm])
        for k in range(3):
            out["spline%d.herm%d" % (i, k)] = float(s["herm"][k])
    return out


# ---- the settings and the input of the device tests ---------------------------------------------------------------------
def channel_settings(ch):
    """Different settings for every channel.  Within a workgroup of four: 0, 1, 2 and 4 splines (ch % 4), and 1, 3, 5, 2
    entries in each reaction table; dots and levels are given in unsorted order; thresholds are distinct.  The levels lie
    inside the range sweep() and compressor_ref.sidechain() pass through."""
    r = np.random.default_rng(3000 + ch)
    nd = (0, 1, 2, 4)[ch % 4]
    nl = (0, 2, 4, 1)[ch % 4]
    db = np.sort(r.uniform(-50.0, -8.0, 4))
    db += np.arange(4) * 3.0                                    # at least 3 dB apart
    dots = [(float(f32(10.0 ** (db[i] / 20.0))), float(f32(10.0 ** ((db[i] * r.uniform(0.5, 0.9) - 3.0) / 20.0))),
             float(f32(10.0 ** (r.uniform(-9.0, -1.0) / 20.0)))) for i in range(4)]
    order = r.permutation(4)
    dots = [dots[i] if k < nd else None for k, i in enumerate(order)]
    lv = [float(f32(10.0 ** (v / 20.0))) for v in (-40.0, -28.0, -16.0, -6.0)]
    perm = r.permutation(4)
    levels = lambda: [lv[i] if k < nl else None for k, i in enumerate(perm)]
    return dict(sample_rate=int(r.choice([44100, 48000, 96000])), hold=float(f32(r.choice([0.0, 0.05, 0.3]))),
                in_ratio=float(f32(r.uniform(1.0, 3.0))), out_ratio=float(f32(r.uniform(1.0, 20.0))), dots=dots,
                attack_levels=levels(), release_levels=levels(),
                attack_times=[float(f32(v)) for v in r.uniform(0.05, 2.0, 5)],
                release_times=[float(f32(v)) for v in r.uniform(0.2, 5.0, 5)])


def sweep(seed, C, n):
    """A rectified tone whose level sweeps from -70 dB to +3 dB and back, twice over n samples, with a little noise: the
    envelope passes every reaction level in both directions."""
    r = np.random.default_rng(seed)
    i = np.arange(n)
    db = -70.0 + 73.0 * np.abs(np.sin(2.0 * np.pi * i / max(n, 2) + r.uniform(0.0, 0.3, (C, 1))))
    x = 10.0 ** (db / 20.0) * np.abs(np.sin(0.9 * i + r.uniform(0.0, 3.0, (C, 1)))) * (1.0 + 0.05 * r.standard_normal((C, n)))
    return x.astype(f32)
