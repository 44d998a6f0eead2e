"""Shared by make_goldens_fiducials.py, test_fiducials_host.py and test_gpu_fiducials.py: the seeded inputs of the
fiducial-undrift cases (tests/golden/fiducials_cases.npz stores only what the reference made of them).

``picked_cases()``: name -> (info, picks, coordinate or None): ``picks`` is a list of per-pick column dicts (frame, x,
y and maybe z) as ``picked_locs`` would hand them over, in the given row order; with a coordinate the case goes through
``_undrift_from_picked_coordinate`` alone (the large ones, to keep the golden file small), else through
``undrift_from_picked``.  ``table_cases()``: name -> (columns, index or None, info, picks, pick_size, undrift_z) for
``undrift_from_fiducials``.
"""
import numpy as np

PICK_LENGTHS = (1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 2 * 8192 + 5)
FRAME_COUNTS = (1, 255, 257, 8192, 8193, 16500)


def info(frames, size=32):
    return [{"Width": size, "Height": size, "Frames": int(frames), "Pixelsize": 130}]


def pick(rng, frames, n_frames, dtype=np.float32, z=False, centre=None, frame_dtype=np.uint32):
    """One fiducial: a common slow drift over the frame number, the pick's own centre and noise."""
    frames = np.asarray(frames)
    t = frames.astype(np.float64) / max(int(n_frames), 1)
    cx, cy = rng.uniform(2, 30, 2) if centre is None else centre
    n = len(frames)
    cols = {"frame": frames.astype(frame_dtype),
            "x": (cx + 0.3 * np.sin(3 * t) + rng.normal(0, 0.02, n)).astype(dtype),
            "y": (cy + 0.2 * t * t + rng.normal(0, 0.02, n)).astype(dtype)}
    if z:
        cols["z"] = (50 * np.cos(2 * t) + rng.normal(0, 5, n)).astype(dtype)
    return cols


def subset(rng, n_frames, n, lo=0, hi=None):
    """n distinct ascending frames of [lo, hi)"""
    hi = n_frames if hi is None else hi
    return np.sort(rng.choice(np.arange(lo, hi), size=n, replace=False))


def picked_cases():
    rng = np.random.default_rng(20261117)
    c = {}
    # the per-pick sum at every seam of NumPy's add.reduce, one pick per length
    F = PICK_LENGTHS[-1]
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        c["lengths_" + name] = (info(F), [pick(rng, subset(rng, F, n), F, dt) for n in PICK_LENGTHS], "x")
    # the row sum's chunk edge and the per-frame grid's tail; holes at the head, the tail and in the middle
    for F in FRAME_COUNTS:
        if F == 1:
            picks = [pick(rng, [0], 1), pick(rng, [0], 1), pick(rng, [0], 1)]
        else:
            lo, hi = F // 50 + 1, F - F // 40 - 2
            picks = []
            for k in range(4):
                f = subset(rng, F, int(0.8 * (hi - lo)), lo, hi)
                picks.append(pick(rng, f[(f < F // 2 - 3) | (f > F // 2 + 2)], F, np.float64 if F == 257 else np.float32))
        c[f"frames_{F}"] = (info(F), picks, "y" if F > 300 else None)
    c["single_covered"] = (info(300), [pick(rng, [137], 300), pick(rng, [137], 300), pick(rng, [137], 300)], None)
    # order: repeated frames, sorted and shuffled; frames that wrap; frames outside
    F = 400
    rep = np.sort(rng.integers(20, 380, 500))
    c["repeats_sorted"] = (info(F), [pick(rng, rep, F), pick(rng, np.sort(rng.integers(0, F, 450)), F), pick(rng, subset(rng, F, 300), F)], None)
    c["repeats_shuffled"] = (info(F), [pick(rng, rng.permutation(rep), F), pick(rng, rng.integers(0, F, 600), F),
                                       pick(rng, rng.permutation(subset(rng, F, 300)), F)], None)
    neg = subset(rng, F, 300).astype(np.int64)
    neg[::3] -= F
    c["negative_frames"] = (info(F), [pick(rng, neg, F, frame_dtype=np.int64), pick(rng, subset(rng, F, 350), F, frame_dtype=np.int64),
                                      pick(rng, np.r_[-F, -1, 5, -1, 7], F, frame_dtype=np.int64)], None)
    c["frame_equal_frames"] = (info(F), [pick(rng, subset(rng, F, 300), F), pick(rng, np.r_[subset(rng, F, 100), F], F)], None)
    c["frame_below_minus_frames"] = (info(F), [pick(rng, np.r_[3, -F - 1, 9], F, frame_dtype=np.int64), pick(rng, subset(rng, F, 100), F, frame_dtype=np.int64)], None)
    # z in all picks, in some, in none
    c["z_all"] = (info(F), [pick(rng, subset(rng, F, 330), F, z=True) for _ in range(5)], None)
    c["z_some"] = (info(F), [pick(rng, subset(rng, F, 330), F, z=k != 2) for k in range(5)], None)
    c["z_all_f64"] = (info(F), [pick(rng, subset(rng, F, 330), F, np.float64, z=True) for _ in range(3)], None)
    # degenerate: an empty pick among full ones, a single pick, two identical picks, a pick with one row, nothing at all
    full = [pick(rng, subset(rng, F, 350), F) for _ in range(3)]
    c["empty_pick"] = (info(F), [full[0], pick(rng, [], F), full[1], full[2]], None)
    c["single_pick"] = (info(F), [full[0]], None)
    c["identical_picks"] = (info(F), [full[1], {k: v.copy() for k, v in full[1].items()}], None)
    c["identical_and_other"] = (info(F), [full[1], {k: v.copy() for k, v in full[1].items()}, full[2]], None)
    c["one_row_pick"] = (info(F), [full[0], pick(rng, [200], F), full[2]], None)
    c["all_empty"] = (info(F), [pick(rng, [], F), pick(rng, [], F)], None)
    return c


def table(rng, n, n_frames, dtype, centres, radius, z=True, per_frame=1.0):
    """A table sorted by frame: fiducials that blink at `centres` over a background cloud."""
    frames, xs, ys = [], [], []
    for cx, cy in centres:
        f = np.flatnonzero(rng.random(n_frames) < 0.9 * per_frame)
        f = np.r_[f, rng.integers(0, n_frames, len(f) // 10)]             # some frames twice: ties inside a pick
        t = f / n_frames
        frames.append(f)
        xs.append(cx + 0.4 * t + rng.normal(0, 0.25 * radius, len(f)))
        ys.append(cy - 0.3 * t * t + rng.normal(0, 0.25 * radius, len(f)))
    frames.append(rng.integers(0, n_frames, n))
    xs.append(rng.uniform(0, 32, n))
    ys.append(rng.uniform(0, 32, n))
    frame, x, y = np.concatenate(frames), np.concatenate(xs), np.concatenate(ys)
    order = np.argsort(frame, kind="stable")
    m = len(frame)
    cols = {"frame": frame[order].astype(np.uint32), "x": x[order].astype(dtype), "y": y[order].astype(dtype),
            "photons": rng.uniform(100, 5000, m).astype(np.float32), "lpx": rng.uniform(0.005, 0.05, m).astype(np.float32),
            "lpy": rng.uniform(0.005, 0.05, m).astype(np.float32)}
    if z:
        cols["z"] = (100 * np.sin(2 * cols["frame"] / n_frames) + rng.normal(0, 20, m)).astype(dtype)
    return cols


def table_cases():
    rng = np.random.default_rng(20261118)
    c = {}
    F = 300
    centres = [(5.0, 5.0), (5.6, 5.3), (20.0, 11.0), (12.5, 27.0)]               # the first two overlap
    picks = [(5.0, 5.0), (5.6, 5.3), (20.0, 11.0), (12.5, 27.0), (40.0, 3.0)]
    t32 = table(rng, 400, F, np.float32, centres, 0.8)
    c["fid_f32"] = (t32, None, info(F), picks, 0.8, True)
    t64 = table(rng, 400, F, np.float64, centres, 0.8)
    c["fid_f64_index"] = (t64, rng.permutation(len(t64["x"])) * 3 + 7, info(F), picks, 0.8, True)
    c["fid_no_z_column"] = (table(rng, 400, F, np.float32, centres, 0.8, z=False), None, info(F), picks[:4], 0.8, True)
    c["fid_undrift_z_false"] = (t32, None, info(F), picks[:4], 0.8, False)
    # insane rows: dropped for the picks, still shifted; a pick without members far from everything
    bad = {k: v.copy() for k, v in t32.items()}
    at = np.flatnonzero((np.abs(bad["x"] - 5.0) < 0.3) & (np.abs(bad["y"] - 5.0) < 0.3))[:6]
    bad["lpx"][at[0]], bad["lpy"][at[1]], bad["photons"][at[2]] = np.nan, np.inf, -1.0
    bad["x"][at[3]], bad["y"][at[4]], bad["x"][at[5]] = -0.5, 40.0, np.nan
    c["fid_insane_rows"] = (bad, None, info(F), picks[:4] + [(100.0, 100.0)], 0.8, True)
    c["fid_int_radius"] = (t32, None, info(F), [(5, 5), (20.0, 11.0), (np.float64(12.5), np.float64(27.0))], 1, True)
    # many rows of a pick in one frame, and holes at both ends
    ties = table(rng, 300, 40, np.float32, centres[2:], 0.8, per_frame=1.0)
    keep = (ties["frame"] > 2) & (ties["frame"] < 36)
    c["fid_tied_frames"] = ({k: v[keep] for k, v in ties.items()}, None, info(40), picks[2:4], 0.8, True)
    # refusals
    c["fid_no_picks"] = (t32, None, info(F), [], 0.8, True)
    c["fid_no_pick_size"] = (t32, None, info(F), picks[:2], None, True)
    c["fid_all_picks_empty"] = (t32, None, info(F), [(100.0, 100.0), (40.0, 3.0)], 0.05, True)
    return c


def generated(n_picks=40, n_frames=20000, coverage=0.95, seed=5):
    """40 picks x 20 000 frames at 95 % coverage -> (offsets, frame int64, [x, y] float32, n_frames), rows by frame."""
    rng = np.random.default_rng(seed)
    picks = [pick(rng, np.flatnonzero(rng.random(n_frames) < coverage), n_frames) for _ in range(n_picks)]
    offsets = np.zeros(n_picks + 1, np.int64)
    offsets[1:] = np.cumsum([len(p["frame"]) for p in picks])
    return offsets, np.concatenate([p["frame"] for p in picks]).astype(np.int64), \
        [np.concatenate([p[k] for p in picks]) for k in ("x", "y")], n_frames


def goldens():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fiducials_cases.npz"))


def frames_of(picks):
    """The per-pick column dicts as the list of DataFrames picked_locs returns."""
    import pandas as pd
    return [pd.DataFrame(dict(p)) for p in picks]


def table_frame(cols, index):
    import pandas as pd
    df = pd.DataFrame(dict(cols))
    if index is not None:
        df.index = index
    return df


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
