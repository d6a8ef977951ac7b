#!/usr/bin/env python3
"""tests/golden/reference_runs/*.npz: numbers computed by the reference's own model programs (oracle/ref_programs.py).

Every case file holds its inputs (model, obs_interval, T, S, R, noise kind, sigma, u, v_0, v_seq, n, y, w, lam) and, from the
programs executed with 50-digit arithmetic and rounded to double,

    z = generate_z(u), x_0 = generate_x_0(z, v_0), sigma_y = generate_sigma_y(u) (variable noise only),
    x_seq [B, T S + 1, X]   x_0 followed by T S applications of forward_func,
    x_obs [B, T, X]         its points at the observation times,
    obs   [B, T, 1]         obs_func there,
    c     [B, T]            obs + sigma n - y,

each with `e_ref64_<name>`: the distance (distance() below: inf-norm over the array, scale max(1, max |value|)) of the same
programs run in double precision from the 50-digit values, measured here.  For the cases with one partition (R >= T) also
J w and J^T lam of c at q = (u, v_0, v_seq, n), as central differences of the 50-digit programs with step 1e-20 (truncation
error about 1e-40; there is no double-precision run of a difference quotient with that step, hence no e_ref64).

usage: generate_reference_runs.py [case ...]    (default: every case and notebook_data.npz)
       generate_reference_runs.py --device-normals [FILE]    (on a machine with the GPU, before the cases: writes
                                                              reference_runs/device_normals.npz, or FILE)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_programs as rp  # noqa: E402

OUT = os.path.join(HERE, "reference_runs")
B = 3
CLIP = -500.0
DIFF_STEP = "1e-20"

# id: model, T, S, R, noise (0 none, 1 fixed sigma, 2 sigma = generate_sigma_y(u)), sigma, obs_interval, seed
CASES = {
    "fhn_3x8": ("fhn", 3, 8, 3, 1, 0.1, 0.2, 11),
    "fhn_9x8": ("fhn", 9, 8, 3, 0, 0.0, 0.2, 12),
    "fhn_3x5": ("fhn", 3, 5, 3, 1, 0.1, 0.2, 13),
    "fhn_nb_4x8": ("fhn_nb", 4, 8, 4, 0, 0.0, 0.5, 14),
    "sir_3x8": ("sir", 3, 8, 3, 1, 1.0, 0.25, 15),
    "sir_3x5": ("sir", 3, 5, 3, 1, 1.0, 0.25, 16),
    "sir_12x8": ("sir", 12, 8, 12, 1, 1.0, 0.25, 17),
    "sir_absorbed": ("sir", 3, 8, 3, 1, 1.0, 0.25, 18),
    "fhn_varsigma_3x8": ("fhn", 3, 8, 3, 2, 0.0, 0.2, 19),
}
U_CENTRE = {"fhn": [-1.2, -2.0, 0.4, 0.8], "fhn_nb": [-0.4, 0.0, 1.0, -0.4], "sir": [-1.0, -1.0, 1.0, 0.0]}
# predict_device's replicates (tests/reference_runs.py PREDICT): the library's keyed normals [B, n_rep, n] of the cases that
# have a prediction, read from the library on an MI355X with ChmcContext.fill_normal -- data, an input of this generator
DEVICE_NORMALS, PREDICT_HORIZON, PREDICT_STRIDE = "device_normals.npz", 1, 1
ABSORB_STEP, ABSORB_LOG_I, ABSORB_LOG_S = 10, -600.0, -499.5  # sir_absorbed: the crafted step and where it lands


def distance(a, ref):
    """max |a - ref| / max(1, max |ref|) over the whole array; inf if `a` is not finite somewhere."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.isfinite(a).all():
        return np.inf
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def draw_inputs(cid):
    """The case's random inputs, doubles: u [B, U], v_0 [B, V0], v_seq [B, T S, V], n [B, T], w [B, Q], lam [B, T]."""
    model, T, S, _, noise, _, _, seed = CASES[cid]
    rng = np.random.default_rng(seed)
    X, V = (3, 3) if model == "sir" else (2, 2)
    V0 = 1 if model == "sir" else 2
    u = np.array(U_CENTRE[model]) + 0.1 * rng.standard_normal((B, 4))
    if noise == 2:
        u = np.concatenate([u, np.log(0.1) + 0.1 * rng.standard_normal((B, 1))], 1)
    v_0 = 1.0 + 0.1 * rng.standard_normal((B, 1)) if model == "sir" else 0.5 * rng.standard_normal((B, 2))
    v_seq = rng.standard_normal((B, T * S, V))
    n = rng.standard_normal((B, T)) if noise else np.zeros((B, 0))
    Q = u.shape[1] + V0 + T * S * V + n.shape[1]
    return dict(u=u, v_0=v_0, v_seq=v_seq, n=n, w=rng.standard_normal((B, Q)), lam=rng.standard_normal((B, T)))


def simulate(m, u, v_0, v_seq, delta, S, noise, sigma, n, y=None, start=None):
    """One chain through the reference's programs in the current number mode.  start = (step k, x_k, z, x_seq so far):
    resume after step k of a path that shares everything before it."""
    u, v_0, v_seq = rp.to_array(u), rp.to_array(v_0), rp.to_array(v_seq)
    if start is None:
        z = m["generate_z"](u)
        x = m["generate_x_0"](z, v_0)
        xs, k0 = [rp.to_array(x)], 0
    else:
        k0, x, z, before = start
        xs = list(before[:k0 + 1])
    for k in range(k0, len(v_seq)):
        x = m["forward_func"](z, x, v_seq[k], delta)
        xs.append(x)
    x_seq = rp.to_array(xs)
    obs = rp.to_array(m["obs_func"](x_seq[S::S]))
    out = dict(z=rp.to_array(z), x_0=x_seq[0], x_seq=x_seq, x_obs=x_seq[S::S], obs=obs)
    sg = None
    if noise == 2:
        sg = out["sigma_y"] = rp.to_array(m["generate_sigma_y"](u))
    elif noise == 1:
        sg = rp.to_array(sigma)
    if y is not None:
        c = obs[:, 0] - rp.to_array(y)
        out["c"] = rp.to_array(c + sg * rp.to_array(n) if noise else c)
    return out


def craft_absorption(m, inp, delta, S):
    """sir_absorbed: two entries of v_seq, both of step ABSORB_STEP, chosen (in double precision) so that this step takes
    log I to ABSORB_LOG_I, below the cutoff, and log S to ABSORB_LOG_S, just above it.  The first-order step is affine in v:
    three evaluations of the reference's own forward_func give the 2 x 2 system."""
    with rp.number_mode("f64"):
        for c in range(B):
            v = inp["v_seq"][c]
            r = simulate(m, inp["u"][c], inp["v_0"][c], v[:ABSORB_STEP], delta, S, 0, 0.0, None)
            z, x = r["z"], r["x_seq"][-1]
            base = np.array(v[ABSORB_STEP])
            f = lambda a, b: np.asarray(m["forward_func"](z, x, np.array([a, b, base[2]]), delta), dtype=np.float64)[:2]  # noqa: E731
            f0 = f(0.0, 0.0)
            A = np.stack([f(1.0, 0.0) - f0, f(0.0, 1.0) - f0], 1)
            v[ABSORB_STEP, :2] = np.linalg.solve(A, np.array([ABSORB_LOG_S, ABSORB_LOG_I]) - f0)


def predict(m, r, W, delta, HS, stride):
    """One chain's replicate futures in the current number mode: from the last point of its path r["x_seq"] over the
    normals W [n_rep, >= HS V] (the step normals come first in a replicate's stream); every stride-th point and obs_func."""
    V = m["dim_v"]
    xs = []
    for w in W:
        x, pts = r["x_seq"][-1], []
        v = rp.to_array(w[:HS * V]).reshape(HS, V)
        for k in range(HS):
            x = m["forward_func"](r["z"], x, v[k], delta)
            if (k + 1) % stride == 0:
                pts.append(x)
        xs.append(rp.to_array(pts))
    xs = rp.to_array(xs)
    return dict(pred_x=xs, pred_obs=rp.to_array(m["obs_func"](xs)))


def to_double(a):
    return np.array([float(t) for t in np.ravel(a)]).reshape(np.shape(a))


def derivatives(m, case, inp, y, base):
    """J w [B, T] and J^T lam [B, Q] by central differences of the 50-digit programs (number mode "mp" is on)."""
    import mpmath
    model, T, S, R, noise, sigma, obs_interval, _ = case
    delta = obs_interval / S
    h = mpmath.mpf(DIFF_STEP)
    Jw, JTl = [], []
    for c in range(B):
        parts = [rp.to_array(inp[k][c]).reshape(-1) for k in ("u", "v_0", "v_seq", "n")]
        q = np.concatenate(parts).view(rp.Arr)
        o1 = len(parts[0])
        o2 = o1 + len(parts[1])
        o3 = o2 + len(parts[2])
        V = inp["v_seq"].shape[2]

        def constr(qq, first_changed=0):
            start = None
            if first_changed >= o2:  # only the noise of step k (or n) differs: resume the base path there
                k = min((first_changed - o2) // V, T * S)
                start = (k, base[c]["x_seq"][k], base[c]["z"], base[c]["x_seq"])
            return simulate(m, qq[:o1], qq[o1:o2], qq[o2:o3].reshape(-1, V), delta, S, noise, sigma, qq[o3:], y, start)["c"]

        w = rp.to_array(inp["w"][c])
        Jw.append((constr(q + h * w) - constr(q - h * w)) / (2 * h))
        lam = rp.to_array(inp["lam"][c])
        g = []
        for i in range(len(q)):
            e = rp.to_array(np.zeros(len(q)))
            e[i] = h
            g.append(((constr(q + e, i) - constr(q - e, i)) * lam).sum() / (2 * h))
        JTl.append(g)
    return to_double(Jw), to_double(JTl)


def generate_case(cid, with_derivatives=True):
    """dict of arrays: what the case's file holds."""
    progs = rp.load()
    case = CASES[cid]
    model, T, S, R, noise, sigma, obs_interval, _ = case
    m = progs.models[model]
    delta = obs_interval / S
    inp = draw_inputs(cid)
    if cid == "sir_absorbed":
        craft_absorption(m, inp, delta, S)
    runs = {}
    y = None
    pred_W = None
    with np.load(os.path.join(OUT, DEVICE_NORMALS)) as f:
        if cid in f.files:
            pred_W = f[cid]
            inp["pred_W"] = pred_W
    for mode in ("f64", "mp"):  # (f64 first: the data y = obs + sigma n of chain 0 are an input, a double)
        with rp.number_mode(mode):
            if y is None:
                r0 = simulate(m, inp["u"][0], inp["v_0"][0], inp["v_seq"][0], delta, S, noise, sigma, inp["n"][0], np.zeros(T))
                y = to_double(r0["c"])
            runs[mode] = [simulate(m, inp["u"][c], inp["v_0"][c], inp["v_seq"][c], delta, S, noise, sigma, inp["n"][c], y)
                          for c in range(B)]
            if pred_W is not None:
                for c in range(B):
                    runs[mode][c].update(predict(m, runs[mode][c], pred_W[c], delta, PREDICT_HORIZON * S, PREDICT_STRIDE))
            if mode == "mp":
                import mpmath
                for r in runs[mode]:
                    assert all(isinstance(t, mpmath.mpf) for a in r.values() for t in np.ravel(a)), "precision lost"
                if cid == "sir_absorbed":
                    check_absorbed(runs[mode], S)
                dv = derivatives(m, case, inp, y, runs[mode]) if with_derivatives and R >= T else None
    out = dict(model=np.array(model), T=np.array(T), S=np.array(S), R=np.array(R), noise=np.array(noise), sigma=np.array(sigma),
               obs_interval=np.array(obs_interval), y=y, **inp)
    for name in runs["mp"][0]:
        ref = np.stack([to_double(r[name]) for r in runs["mp"]])
        out[name] = ref
        out["e_ref64_" + name] = np.array(distance(np.stack([to_double(r[name]) for r in runs["f64"]]), ref))
    if dv is not None:
        out["Jw"], out["JTlam"] = dv
    for k, v in out.items():
        assert v.dtype.kind == "U" or np.isfinite(v).all(), (cid, k)
    return out


def check_absorbed(runs, S):
    """Conditions on the 50-digit run alone: no component within 1e-6 of the cutoff unless it sits on it exactly (the
    clipped state the reference's select hands on), log I clipped from the step after the crafted one to the end, log S
    never clipped."""
    for r in runs:
        xs = to_double(r["x_seq"])
        off = np.abs(xs[:, :2] - CLIP)
        assert ((off == 0) | (off > 1e-6)).all()
        assert xs[ABSORB_STEP + 1, 1] < CLIP and (xs[ABSORB_STEP + 2:, 1] == CLIP).all() and (xs[:ABSORB_STEP + 1, 1] > CLIP).all()
        assert (xs[:, 0] > CLIP).all() and CLIP < xs[ABSORB_STEP + 1, 0] < CLIP + 1.0
        assert ABSORB_STEP + 2 < len(xs) - S  # clipped for more than a whole observation interval


def notebook_data():
    """The notebook's own data cells, run in double precision when it was loaded: the head of q_ref, z, x_0, y_seq_ref; and
    its generate_from_model on the same q_ref with 50-digit arithmetic (`*_mp`, with the distances e_ref64_* of the former)."""
    nb = rp.load().nb
    out = dict(T=np.array(nb["num_obs"]), S=np.array(nb["num_steps_per_obs"]), obs_interval=np.array(nb["obs_interval"]),
               q_ref_head=np.asarray(nb["q_ref"][:16], dtype=np.float64), q_ref_sum=np.array(float(np.sum(nb["q_ref"]))),
               z=np.asarray(nb["z_ref"], dtype=np.float64), x_0=np.asarray(nb["x_0_ref"], dtype=np.float64),
               y_seq_ref=np.asarray(nb["y_seq_ref"], dtype=np.float64))
    with rp.number_mode("mp"):
        _, y, z, x_0 = nb["generate_from_model"](rp.to_array(nb["q_ref"]), rp.to_array(nb["δ"]).item(), nb["dim_x"], nb["dim_z"],
                                                 nb["dim_v"], nb["num_steps_per_obs"])
        for name, v in (("y_seq_ref", y), ("z", z), ("x_0", x_0)):
            out[name + "_mp"] = to_double(v)
            out["e_ref64_" + name] = np.array(distance(out[name], out[name + "_mp"]))
    return out


def write_device_normals(path):
    """On a machine with the GPU: the library's keyed normals of the predict call of every case that has a prediction."""
    sys.path.insert(0, os.path.dirname(HERE))
    import reference_runs as rr
    out = {}
    for cid in rr.PREDICT_CASES:
        ctx = rr.make_ctx(cid)
        assert ctx.on_gpu, "the normals the device tests are held to come from the device library"
        steps = PREDICT_HORIZON * ctx.S
        out[cid] = rr.predict_normals(ctx, steps * ctx.V + (steps // PREDICT_STRIDE if ctx.noisy else 0))
        ctx.close()
    np.savez(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


def main(names):
    os.makedirs(OUT, exist_ok=True)
    if names[:1] == ["--device-normals"]:
        return write_device_normals(names[1] if len(names) > 1 else os.path.join(OUT, DEVICE_NORMALS))
    for cid in names or list(CASES) + ["notebook_data"]:
        data = notebook_data() if cid == "notebook_data" else generate_case(cid)
        path = os.path.join(OUT, cid + ".npz")
        np.savez_compressed(path, **data)
        print(cid, os.path.getsize(path), "bytes", {k: f"{float(v):.1e}" for k, v in data.items() if k.startswith("e_ref64")})


if __name__ == "__main__":
    main(sys.argv[1:])
