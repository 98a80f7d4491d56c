"""What tests/test_dynamics_reference_host.py and tests/test_dynamics_reference_gpu.py share: the recorded results of the
reference's own Compressor, Expander, Gate and DynamicProcessor (tests/golden/dynamics_ref_vectors.npz, written by
tests/golden/make_dynamics_vectors.py) in the shapes the restatements take, the restatements' followers run over a recorded
case, and their derived gain bounds applied to a recorded or a computed gain."""
import os
import sys

import numpy as np

import compressor_ref as cr
import dynproc_ref as dr
import expander_ref as er
import gate_ref as gr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_dynamics_vectors as mv  # noqa: E402

f32 = np.float32
CLASSES = mv.CLASSES
U = cr.U
same = mv.same
bits = mv.bits


def load():
    return mv.load()


# ---- parameters: recorded rows <-> the dicts of get_params / compute_params ---------------------------------------------
def params_dict(cls, paramf, parami):
    p = {k: f32(v) for k, v in zip(mv.PARAMF[cls], np.asarray(paramf, f32))}
    i = {k: int(v) for k, v in zip(mv.PARAMI[cls], parami)}
    if cls == "compressor":
        return {"tau_attack": p["tau_attack"], "tau_release": p["tau_release"], "release_threshold": p["release_threshold"], "hold": i["hold"],
                "k": [{"start": p["k%d.start" % j], "end": p["k%d.end" % j], "gain": p["k%d.gain" % j],
                       "herm": np.array([p["k%d.herm%d" % (j, n)] for n in range(3)], f32),
                       "tilt": np.array([p["k%d.tilt%d" % (j, n)] for n in range(2)], f32)} for j in range(2)]}
    if cls == "expander":
        return {"tau_attack": p["tau_attack"], "tau_release": p["tau_release"], "release_threshold": p["release_threshold"], "hold": i["hold"],
                "upward": i["upward"],
                "k": {"start": p["start"], "end": p["end"], "threshold": p["threshold"],
                      "herm": np.array([p["herm%d" % n] for n in range(3)], f32), "tilt": np.array([p["tilt%d" % n] for n in range(2)], f32)}}
    if cls == "gate":
        return {"tau_attack": p["tau_attack"], "tau_release": p["tau_release"], "hold": i["hold"],
                "k": [{"start": p["k%d.start" % j], "end": p["k%d.end" % j], "gain_start": p["k%d.gain_start" % j],
                       "gain_end": p["k%d.gain_end" % j], "herm": np.array([p["k%d.herm%d" % (j, n)] for n in range(4)], f32)}
                      for j in range(2)]}
    return {"hold": i["hold"],
            "attack": [{"level": p["attack%d.level" % n], "tau": p["attack%d.tau" % n]} for n in range(i["attacks"])],
            "release": [{"level": p["release%d.level" % n], "tau": p["release%d.tau" % n]} for n in range(i["releases"])],
            "splines": [dict([(k, p["spline%d.%s" % (n, k)]) for k in mv._SPLINE[:6]] +
                             [("herm", np.array([p["spline%d.herm%d" % (n, m)] for m in range(3)], f32))]) for n in range(i["splines"])]}


def flat(cls, p):
    """A get_params / compute_params dict as (float32 row, integer row) in the recorded layout."""
    if cls == "compressor":
        f = [p["tau_attack"], p["tau_release"], p["release_threshold"]]
        for k in p["k"]:
            f += [k["start"], k["end"], k["gain"]] + list(k["herm"][:3]) + list(k["tilt"][:2])
        i = [p["hold"]]
    elif cls == "expander":
        k = p["k"]
        f = [p["tau_attack"], p["tau_release"], p["release_threshold"], k["start"], k["end"], k["threshold"]] + list(k["herm"][:3]) + list(k["tilt"][:2])
        i = [p["hold"], 1 if p["upward"] else 0]
    elif cls == "gate":
        f = [p["tau_attack"], p["tau_release"]]
        for k in p["k"]:
            f += [k["start"], k["end"], k["gain_start"], k["gain_end"]] + list(k["herm"][:4])
        i = [p["hold"]]
    else:
        f = []
        for name in ("attack", "release"):
            for n in range(5):
                f += [p[name][n]["level"], p[name][n]["tau"]] if n < len(p[name]) else [0.0, 0.0]
        for n in range(4):
            if n < len(p["splines"]):
                s = p["splines"][n]
                f += [s[k] for k in mv._SPLINE[:6]] + list(s["herm"][:3])
            else:
                f += [0.0] * 9
        i = [p["hold"], len(p["splines"]), len(p["attack"]), len(p["release"])]
    return np.array(f, f32), np.array(i, np.uint32)


def settings(case):
    return mv.settings_dict(case["cls"], case["settings"])


def written(case):
    """The state a subclass wrote after the first call, or None: (e, peak, hold, curve)."""
    w = case["write"]
    if not w[0]:
        return None
    return w[1:2].view(f32)[0], w[2:3].view(f32)[0], int(w[3]), int(w[4])


# ---- the restatements' followers over a recorded case -------------------------------------------------------------------
def follow(case, params):
    """The restatement's follower of the case's class fed `params`, call by call, a written state taken in after the first:
    (env [n], which [n] or None, states uint32 [calls, 4] as recorded, counters)."""
    cls = case["cls"]
    x = np.ascontiguousarray(case["x"], f32)[None, :]
    st = gr.fresh_state(1) if cls == "gate" else (dr.fresh_state(1) if cls == "dynproc" else cr.fresh_state(1))
    envs, whichs, states, total = [], [], [], {}
    stats = gr.fresh_stats()
    pos = 0
    with np.errstate(all="ignore"):
        for ci, n in enumerate(case["calls"]):
            part = x[:, pos:pos + n]
            pos += n
            if cls in ("compressor", "expander"):
                env, taken = cr.follow(part, st, [params["tau_attack"]], [params["tau_release"]], [params["release_threshold"]], [params["hold"]])
            elif cls == "dynproc":
                env, taken = dr.follow(part, st, [params])
                taken = {k: taken[k] for k in dr.BRANCHES}
            else:
                env, which = gr.process(part, st, [params["tau_attack"]], [params["tau_release"]], [params["hold"]],
                                        [params["k"][0]["end"]], [params["k"][1]["start"]], stats)
                whichs.append(which[0])
                taken = {}
            for k, v in taken.items():
                total[k] = total.get(k, 0) + v
            envs.append(env[0])
            states.append([bits(st["e"])[0], bits(st["peak"])[0], int(st["hold"][0]), int(st["curve"][0]) if cls == "gate" else 0])
            w = written(case)
            if ci == 0 and w is not None:
                st["e"], st["peak"], st["hold"] = np.array([w[0]], f32), np.array([w[1]], f32), np.array([w[2]], np.uint32)
                if cls == "gate":
                    st["curve"] = np.array([w[3]], np.uint32)
    if cls == "gate":
        total = {k: stats[k] for k in ("toggles", "capped", "restep_hold")}
    return np.concatenate(envs), (np.concatenate(whichs) if whichs else None), np.array(states, np.uint32), total


# ---- the restatements' float64 curves and derived bounds ----------------------------------------------------------------
GAIN_KIND = {"compressor": "reduction", "expander": "amplification", "gate": "amplification", "dynproc": "reduction"}


def expected(cls, kind, level, params, which=None, scalar=False, either_branch=False):
    """The float64 value, the derived bound in u and where the result is exact, for one overload on `level` [n]:
    kind is one of mv.CURVES[cls] ("curve0" / "amplification1": Gate's hyst), or "gain" for what process() writes.
    either_branch: the bound for a logf other than this machine's (dynproc_ref.gain_bound_either; DynamicProcessor alone
    chooses its branches on the logarithm, the other three on the level)."""
    level = np.ascontiguousarray(level, f32)[None, :]
    P = [params]
    with np.errstate(all="ignore"):
        if cls == "compressor":
            # the array reduction() is the curve; the scalar one, and process(), the gain
            scaled = kind == "curve" or (kind == "reduction" and not scalar)
            g, b = cr.gain64(level, P), cr.gain_bound(level, P)
            exact = np.zeros(g.shape, bool)
            if scaled:
                g, b = g * np.abs(level).astype(np.float64), b + 1.0
        elif cls == "expander":
            g, b = er.gain64(level, P), er.gain_bound(level, P)
            exact = b == 0
            if kind == "curve":
                g, b = g * er.limited(level, P).astype(np.float64), b + 1.0
        elif cls == "gate":
            if which is None:
                which = np.full(level.shape, 1 if kind.endswith("1") else 0, np.uint32)
            which = np.asarray(which).reshape(level.shape)
            g, b = gr.gain64(level, which, P), gr.gain_bound(level, which, P)
            exact = b == 0
            if kind.startswith("curve"):
                g, b, exact = g * np.abs(level).astype(np.float64), b + 1.0, np.zeros(g.shape, bool)
        else:
            model = kind == "model"
            lo = dr.GAIN_AMP_MIN if kind == "gain" or (kind == "reduction" and not scalar) else dr.FLOAT_SAT_M_INF
            g = dr.gain64(level, P, lo=lo, model=model)
            b = (dr.gain_bound_either if either_branch else dr.gain_bound)(level, P, lo=lo, model=model)
            exact = np.full(g.shape, len(params["splines"]) == 0)
            if kind in ("curve", "model"):
                g = g * dr.limited(level, lo).astype(np.float64)
                b = b + 1.0
    return g[0], b[0], exact[0]


def judge(got, g64, bound, exact, factor=1.0):
    """got (float32) against the float64 value under factor x the bound: (ok per sample, error in u).  Exact where the
    restatement says the result is a stored constant; elsewhere dynproc_ref.within(), which also states what a bound in u
    means for a result below the smallest normal float32 or above the largest."""
    got64 = np.asarray(got, np.float64)
    ok, err = dr.within(got64, np.abs(g64), factor * bound)
    with np.errstate(all="ignore"):
        zero = g64 == 0
        ok = np.where(zero, got64 == 0, ok)
        ok = np.where(exact, got64 == g64, ok)
        err = np.where(zero | exact, 0.0, err)
    return ok, err


def judge_pair(got, ref, g64, tol, exact=None):
    """Two float32 evaluations of the same curve against each other: each lies within its derived bound of the float64 value
    g64, so they differ by at most the sum `tol` (in u) of the two bounds, relative to g64: the triangle inequality, no fitted
    factor.  Below the smallest normal float32 a bound in u is meant at that number plus one subnormal spacing per side; above
    the largest both sides are at it or infinite.  Where the result is a stored constant (`exact`) the two are equal.
    (ok per sample, difference in u)."""
    got, ref, g64 = (np.abs(np.asarray(v, np.float64)) for v in (got, ref, g64))
    tiny, huge = 2.0 ** -126, float(np.finfo(f32).max)
    with np.errstate(all="ignore"):
        diff = np.abs(got - ref)
        scale = U * np.maximum(g64, tiny)
        ok = diff <= tol * scale + np.where(g64 < tiny, 2.0 * 2.0 ** -149, 0.0)
        ok = np.where(g64 > huge, (got == ref) | (got >= huge * (1.0 - tol * U)), ok)
        if exact is not None:
            ok = np.where(exact, got == ref, ok)
        err = np.where(g64 > huge, 0.0, diff / scale)
    return ok, err


def case_for_driver(c):
    """A loaded case as make_dynamics_vectors.case_bytes() takes it."""
    w = written(c)
    return dict(cls=c["cls"], name=c["name"], settings=np.asarray(c["settings"], f32), x=np.asarray(c["x"], f32), calls=list(c["calls"]),
                write=w, write_after=1, ladder=np.asarray(c.get("ladder", np.zeros(0, f32)), f32))


def pair_tolerance(cls, kind, level, params, which=None, scalar=False, direct=True):
    """(float64 value, tolerance in u, exact) for a device result: against the reference's recorded float32 result (direct) the
    sum of the two derived bounds, the reference's with this machine's logf and the device's with its own; against the
    float64 value alone (fallback) the device's."""
    g64, b_dev, exact = expected(cls, kind, level, params, which, scalar, either_branch=True)
    if not direct:
        return g64, b_dev, exact
    return g64, b_dev + expected(cls, kind, level, params, which, scalar)[1], exact
