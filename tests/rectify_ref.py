"""NumPy restatement of history rectification (include/lrt.h, lrt_temporal_rectify_*), the cases its
tests share and the sequences that show what it is for. A helper module, not a conftest: imported by
tests/test_rectify_cpu.py and tests/test_gpu_rectify.py.

Per pixel p, with i = id(p), r(q) = ref_scale ref(q).rgb, K = r(p), c and M the state's color and
moment2 rgb and n moment2's alpha:
  1. the window q = p + (dx, dy), |dx|, |dy| <= radius; a tap counts iff it is inside the image and
     id(q) = i; m = the count; S1 = sum (r(q) - K), S2 = sum (r(q) - K)^2 over the counting taps (a
     select: a tap that does not count adds 0 whatever it holds), row by row, left to right;
     a = S1 / m, mu = K + a, sigma = sqrt(max(S2 / m - a^2, 0))
  2. supported iff m >= min_taps; an unsupported pixel passes c, M and n through (class 2)
  3. lo = mu - gamma sigma, hi = mu + gamma sigma, c' = min(max(c, lo), hi)
  4. moved = (c' != c), d = |c' - c|, t = d / (d + gamma sigma + range_floor), e = max(t)^2,
     n' = n + e (min(n, reset_history) - n); M' = c'^2 + max(M - c^2, 0) on a moved channel, else M;
     class 1 if any channel moved, else 0
  5. std = sqrt(max(M' - c'^2, 0)), or short_std where n' < min_history
`fragile` marks the supported pixels one of whose channels has c within FRAGILE_REL of lo or hi
(temporal_ref._near: every output and the class depend on that decision) and the pixels whose n'
lies that close to min_history (color_std).

`python tests/rectify_ref.py` prints the largest gap between the f32 and the f64 run over the GPU
test's cases (F32_F64_GAP* of tests/test_gpu_rectify.py) with the share of fragile pixels per case;
the ids come from tests/gbuffer_ref.py's f32 run and the colours from the oracle there, from the
library on the GPU.
"""
import numpy as np

import gbuffer_ref as G
import temporal_gbuffer_ref as TG
import temporal_ref as R

DEFAULTS = dict(radius=2, min_taps=5, min_history=4, ref_scale=1.0, gamma=1.0, range_floor=1e-4, reset_history=1.0,
                short_std=1e3)
OUTPUTS = ("color", "moment2", "n", "color_std")
RADII = (1, 2, 3)
MAX_FRAGILE = 0.02
CUR_SCALE, FRAME0 = TG.CUR_SCALE, TG.FRAME0


def step(ref, ids, state, dtype=np.float64, info=None, **params):
    """One call. ref [h, w, >= 3]; ids [h, w]; state {"color", "moment2" (n in its alpha)}. Arithmetic
    in `dtype`. Returns (outputs, fragile): outputs maps OUTPUTS to [h, w, 3] arrays ("n": [h, w]).
    info: a dict to fill with the per-pixel decisions: m, supported, moved [h, w, 3], class, mu,
    sigma [h, w, 3] and e."""
    p = dict(DEFAULTS, **params)
    T = dtype
    rad = int(p["radius"])
    with np.errstate(all="ignore"):
        r = T(p["ref_scale"]) * np.asarray(ref)[..., :3].astype(T)
        ids = np.asarray(ids).astype(np.int64)
        c = np.asarray(state["color"])[..., :3].astype(T)
        M = np.asarray(state["moment2"])[..., :3].astype(T)
        n = np.asarray(state["moment2"])[..., 3].astype(T)
        h, w = ids.shape
        ys, xs = np.mgrid[0:h, 0:w]
        m = np.zeros((h, w), np.int64)
        s1, s2 = np.zeros((h, w, 3), T), np.zeros((h, w, 3), T)
        for dy in range(-rad, rad + 1):
            for dx in range(-rad, rad + 1):
                qx, qy = xs + dx, ys + dy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                counts = inside & (ids[cy, cx] == ids)
                e = np.where(counts[..., None], r[cy, cx] - r, T(0))
                m += counts
                s1 += e
                s2 += e * e
        fm = m.astype(T)[..., None]
        a = s1 / fm
        mu = r + a
        sigma = np.sqrt(np.maximum(s2 / fm - a * a, T(0)))
        gs = T(p["gamma"]) * sigma
        lo, hi = mu - gs, mu + gs
        supported = m >= int(p["min_taps"])
        sup = supported[..., None]
        # fminf(fmaxf(c, lo), hi): a NaN bound is ignored
        cl = np.fmin(np.fmax(c, lo), hi)
        moved = sup & (cl != c)
        d = np.abs(cl - c)
        t = np.where(sup, d / (d + gs + T(p["range_floor"])), T(0))
        e = np.fmax(np.fmax(t[..., 0], t[..., 1]), t[..., 2])
        e = np.fmax(e, T(0)) ** 2
        col = np.where(moved, cl, c)
        m2 = np.where(moved, cl * cl + np.maximum(M - c * c, T(0)), M)
        any_moved = moved.any(-1)
        nn = np.where(any_moved, n + e * (np.minimum(n, T(p["reset_history"])) - n), n)
        cls = np.where(supported, any_moved.astype(np.int32), 2).astype(np.int32)
        fragile = supported & (R._near(c, lo) | R._near(c, hi)).any(-1)
        fragile |= R._near(nn, T(p["min_history"]))
        std = np.sqrt(np.maximum(m2 - col * col, T(0)))
        std = np.where((nn < T(p["min_history"]))[..., None], T(p["short_std"]), std)
    if info is not None:
        info.update({"m": m, "supported": supported, "moved": moved, "class": cls, "mu": mu, "sigma": sigma,
                     "e": np.where(any_moved, e, T(0))})
    return dict(color=col, moment2=m2, n=nn, color_std=std), fragile


def as_state(out, dtype=np.float32):
    """A call's outputs as the two [h, w, 4] buffers a temporal step or the next call takes."""
    return TG.as_state(out, dtype)


def outputs_of(state):
    """A library state {"color", "moment2", "color_std"} as OUTPUTS."""
    return dict(color=state["color"][..., :3], moment2=state["moment2"][..., :3], n=state["moment2"][..., 3],
                color_std=state["color_std"][..., :3])


def count_m(ids, radius):
    """m of step 1 pixel by pixel, in plain loops: the check of step()'s window."""
    h, w = ids.shape
    m = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            for qy in range(max(y - radius, 0), min(y + radius, h - 1) + 1):
                for qx in range(max(x - radius, 0), min(x + radius, w - 1) + 1):
                    m[y, x] += ids[qy, qx] == ids[y, x]
    return m


def gaps(a, fa, b, fb, worst):
    """The f32 - f64 (or got - f64) gaps of one case folded into worst = {"all", "std"}."""
    TG.gaps(a, fa, b, fb, worst)


# ---- the rendered cases of tests/test_gpu_rectify.py::test_call_vs_restatement
def case_list():
    """[(label, w, h, count, radius)]: temporal_gbuffer_ref's shapes and sphere counts at each radius."""
    return [(f"{label} r{rad}", w, h, count, rad) for label, w, h, count in TG.case_list() for rad in RADII]


def rendered_inputs(w, h, count, scene_of, make_camera, planes, colour):
    """(ref, ids, state) of one rendered case, the same at every radius: the ids of the G-buffer of
    the default view, one fresh 1 spp frame (sample FRAME0 into zeroed buffers: ref_scale = CUR_SCALE)
    and temporal_gbuffer_ref.random_state. scene_of, planes and colour as
    temporal_gbuffer_ref.rendered_case takes them."""
    spheres, mats = scene_of(count)
    sph = G.sphere_array(spheres)
    cam, _ = G.camera_pair(make_camera, w, h)
    ids = np.ascontiguousarray(planes(w, h, cam, sph, mats, None, None)["id"], np.int32)
    ref = colour(w, h, cam, sph, mats, FRAME0)
    return ref, ids, TG.random_state(w, h, 1000 * w + h + count)


def rendered_gap(scene_of, make_camera, planes, colour):
    """(all outputs but color_std, color_std, {case: fragile share}) of the f32 - f64 gap over case_list()."""
    worst, shares, inputs = {"all": 0.0, "std": 0.0}, {}, {}
    for label, w, h, count, rad in case_list():
        if (w, h, count) not in inputs:
            inputs[(w, h, count)] = rendered_inputs(w, h, count, scene_of, make_camera, planes, colour)
        args = inputs[(w, h, count)]
        a, fa = step(*args, np.float32, ref_scale=CUR_SCALE, radius=rad)
        b, fb = step(*args, np.float64, ref_scale=CUR_SCALE, radius=rad)
        shares[label] = float(fb.mean())
        gaps(a, fa, b, fb, worst)
    return worst["all"], worst["std"], shares


# ---- the designed cases: 12 x 8 planes written by hand so that each branch of the rule holds pixels
DESIGNED_SIZE = (12, 8)
DESIGNED_CASES = ("step", "inside", "two_ids", "two_ids_min_taps_1", "borders_r1", "borders_r2", "borders_r3", "miss",
                  "reset_history", "min_history", "gamma_0")
# "step": n' - reset_history = (n - reset_history) (1 - e) with 1 - e = 1 - t^2 <= 2 range_floor / d
# at sigma = 0, so n' lies within N_TOL = 1e-3 of reset_history once d >= 2e-4 x 39 / 1e-3 = 7.8
STEP_A, STEP_B, STEP_N, N_TOL = (0.25, 0.5, 1.0), (16.0, 12.0, 9.5), 40.0, 1e-3
ISOLATED = (4, 3)      # (y, x) of two_ids' pixel of a third id
TWO_IDS_REF = (0.25, 1.0, 0.75)    # the constant references of id 0 (left), id 1 (right) and the isolated pixel
TWO_IDS_STATE = 0.5


def _noisy_ref(rng, h, w):
    ref = np.zeros((h, w, 4), np.float32)
    ref[..., :3] = rng.gamma(4.0, 0.25, (h, w, 3))
    return ref


def designed_inputs(case, seed=0):
    """(ref, ids, state, params, expect) of one designed case. expect maps a name to a tuple whose
    first member is a mask [h, w]; both tests read it:
      "m": (mask, m) and "class": (mask, class): the restatement's info, exactly
      "color_is": (mask, [h, w, 3] float32): the colour that comes out, bit for bit
      "passthrough": (mask,): color, moment2 and n come out as they went in, bit for bit
      "n_near": (mask, value, tol); "n_is": (mask, value), exactly
      "short": (mask, bool): color_std is short_std there (True) or below it (False)
    By default the ids are all 0, the reference is noisy (gamma-distributed, mean 1, relative sigma
    0.5) and the state is temporal_gbuffer_ref.random_state."""
    w, h = DESIGNED_SIZE
    k = DESIGNED_CASES.index(case)
    rng = np.random.default_rng([seed, k])
    ref = _noisy_ref(rng, h, w)
    ids = np.zeros((h, w), np.int32)
    state = TG.random_state(w, h, 91 + k)
    params, expect = {}, {}
    every = np.ones((h, w), bool)
    ys, xs = np.mgrid[0:h, 0:w]

    def flat_state(colour, n):
        state["color"][..., :3] = np.float32(colour)
        state["moment2"][..., :3] = state["color"][..., :3] ** 2 + np.float32(0.125)
        state["moment2"][..., 3] = n

    if case == "step":             # a history at A, a noise-free frame at B: one step there, the history gone
        flat_state(STEP_A, STEP_N)
        ref[..., :3] = np.float32(STEP_B) / np.float32(2)
        params = dict(ref_scale=2.0)
        expect = {"class": (every, 1), "color_is": (every, np.broadcast_to(np.float32(STEP_B), (h, w, 3))),
                  "n_near": (every, 1.0, N_TOL), "short": (every, True)}
    elif case == "inside":         # the state's colour is the window's own mean: nothing moves
        info = {}
        step(ref, ids, state, np.float64, info=info)
        state["color"][..., :3] = info["mu"]
        state["moment2"][..., :3] = state["color"][..., :3] ** 2 + np.float32(0.125)
        expect = {"class": (every, 0), "passthrough": (every,)}
    elif case in ("two_ids", "two_ids_min_taps_1"):
        right = xs >= w // 2
        lone = np.zeros((h, w), bool)
        lone[ISOLATED] = True
        ids[right], ids[lone] = 1, 2
        ref[..., :3] = np.where(right, TWO_IDS_REF[1], TWO_IDS_REF[0])[..., None]
        ref[lone, :3] = TWO_IDS_REF[2]
        flat_state(TWO_IDS_STATE, 12.0)
        want = np.float32(ref[..., :3])
        if case == "two_ids":
            expect = {"class": (every, np.where(lone, 2, 1)), "color_is": (~lone, want), "passthrough": (lone,),
                      "m": (lone, 1)}
        else:
            params = dict(min_taps=1)
            expect = {"class": (every, 1), "color_is": (every, want)}
    elif case.startswith("borders"):
        rad = int(case[-1])
        params = dict(radius=rad, min_taps=1)
        mx = np.minimum(xs, rad) + np.minimum(w - 1 - xs, rad) + 1
        my = np.minimum(ys, rad) + np.minimum(h - 1 - ys, rad) + 1
        m = mx * my
        assert m[0, 0] == (rad + 1) ** 2 and m[0, w // 2] == (rad + 1) * (2 * rad + 1) and m.max() == (2 * rad + 1) ** 2
        expect = {"m": (every, m)}
    elif case == "miss":           # misses on the left match misses, and nothing else
        left = xs < w // 2
        ids[left] = -1
        mx = np.where(left, np.minimum(xs, 2) + np.minimum(w // 2 - 1 - xs, 2) + 1,
                      np.minimum(xs - w // 2, 2) + np.minimum(w - 1 - xs, 2) + 1)
        my = np.minimum(ys, 2) + np.minimum(h - 1 - ys, 2) + 1
        expect = {"m": (every, mx * my)}
    elif case == "reset_history":  # a history already shorter than reset_history stays as long as it is
        flat_state(STEP_A, 3.0)
        ref[..., :3] = np.float32(STEP_B)
        params = dict(reset_history=8.0)
        expect = {"class": (every, 1), "n_is": (every, 3.0), "short": (every, True)}
    elif case == "min_history":    # clamped on the left (n' near 1: short_std), inside on the right (n = 10: its own std)
        info = {}
        step(ref, ids, state, np.float64, info=info)
        left = xs < w // 2
        state["color"][..., :3] = np.where(left[..., None], np.float32(40.0), info["mu"])
        state["moment2"][..., :3] = state["color"][..., :3] ** 2 + np.float32(0.125)
        state["moment2"][..., 3] = 10.0
        expect = {"class": (every, np.where(left, 1, 0)), "short": (every, left), "n_is": (~left, 10.0)}
    elif case == "gamma_0":        # the box is the mean itself
        params = dict(gamma=0.0)
        expect = {"class": (every, 1), "color_is_mu": (every,)}
    else:
        raise ValueError(f"unknown designed case {case!r}")
    return ref, ids, state, params, expect


def designed_gap():
    """(all outputs but color_std, color_std, {case: fragile share}) of the f32 - f64 gap over the designed cases."""
    worst, shares = {"all": 0.0, "std": 0.0}, {}
    for case in DESIGNED_CASES:
        ref, ids, state, params, _ = designed_inputs(case)
        a, fa = step(ref, ids, state, np.float32, **params)
        b, fb = step(ref, ids, state, np.float64, **params)
        shares[case] = float(fb.mean())
        gaps(a, fa, b, fb, worst)
    return worst["all"], worst["std"], shares


NAN_AT = (4, 3)        # (y, x) of the non-finite reference value


def nan_ref_inputs(own_id):
    """(ref with a NaN at NAN_AT, the same with 0 there, ids, state): own_id False: NAN_AT is two_ids'
    isolated pixel, a tap of another id for everyone else; True: one id everywhere (gamma_0's noisy
    reference and random state)."""
    ref, ids, state, _, _ = designed_inputs("gamma_0" if own_id else "two_ids")
    if not own_id:
        ref[..., :3] = _noisy_ref(np.random.default_rng(5), *ref.shape[:2])[..., :3]
    zeroed = ref.copy()
    zeroed[NAN_AT][:3] = 0
    ref[NAN_AT][:3] = np.nan
    return ref, zeroed, ids, state


# ---- what it is for, derivable: a noise-free sequence through temporal_gbuffer_ref.step
SEQ_SIZE = (12, 8)
SEQ_A, SEQ_B, SEQ_BEFORE, SEQ_AFTER = 1.0, 17.0, 40, 5


def sequence_planes():
    """(cur, prev_g) of the sequence: one id, one normal, zero motion."""
    w, h = SEQ_SIZE
    cur = {"normal": TG.quad(np.broadcast_to(np.float32(TG.UP), (h, w, 3))), "motion": np.zeros((h, w, 4), np.float32),
           "id": np.zeros((h, w), np.int32)}
    cur["motion"][..., 3] = 1
    return cur, {"normal": cur["normal"].copy(), "id": cur["id"].copy()}


def sequence_frame(value):
    w, h = SEQ_SIZE
    f = np.zeros((h, w, 4), np.float32)
    f[..., :3] = value
    return f


def derivable_sequence(rectify, dtype=np.float64):
    """SEQ_BEFORE frames of SEQ_A, then SEQ_AFTER of SEQ_B, through temporal_gbuffer_ref.step and, if
    `rectify`, step() on the frame itself after every temporal step. Returns [(error, n)] of the
    frames of B: max |color - B| and the n of pixel (0, 0)."""
    cur, prev_g = sequence_planes()
    state, out = None, []
    for k in range(SEQ_BEFORE + SEQ_AFTER):
        frame = sequence_frame(SEQ_A if k < SEQ_BEFORE else SEQ_B)
        o, _ = TG.step(frame, cur, prev_g if state is not None else None, state, dtype)
        state = TG.as_state(o, dtype)
        if rectify:
            o, _ = step(frame, cur["id"], state, dtype)
            state = as_state(o, dtype)
        if k >= SEQ_BEFORE:
            out.append((float(np.abs(o["color"] - SEQ_B).max()), float(o["n"][0, 0])))
    return out


# ---- what it is for, rendered: the default scene's light dimmed under a static camera
DIM = dict(w=67, h=45, steps=12, after=4, light=8, factor=0.25, truth_spp=256)


def dimmed_chain(render, ids, accumulate, rectify):
    """The two chains of the rendered purpose test. render(t, dimmed) -> one fresh 1 spp frame of
    step t ([h, w, 4], sample t into zeroed buffers: cur_scale = t + 1); accumulate(frame, state,
    cur_scale) -> the next plain state; rectify(frame, state, cur_scale) -> the rectified one. Returns
    [(plain colour, rectified colour)] per step, rgb."""
    plain = rect = None
    out = []
    for t in range(DIM["steps"] + DIM["after"]):
        frame, k = render(t, t >= DIM["steps"]), float(t + 1)
        plain = accumulate(frame, plain, k)
        rect = rectify(frame, accumulate(frame, rect, k), k)
        out.append((plain["color"][..., :3].copy(), rect["color"][..., :3].copy()))
    return out


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    from learnraytracing_amd import default_scene, make_camera, random_scene

    for title, (gap, gap_std, shares) in (
            ("rendered", rendered_gap(TG.scene_of(default_scene, random_scene), make_camera, TG.cpu_planes, TG.cpu_colour)),
            ("designed", designed_gap())):
        print(f"largest f32 - f64 gap over the {title} cases: {gap:.3g} (color_std: {gap_std:.3g})")
        for label, s in shares.items():
            print(f"  {label}: fragile {100 * s:.2f} %")
