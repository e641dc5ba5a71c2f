"""Plain numpy restatement of dim_track_visibility and dim_track_update_occ (include/deepim_hip.h), written from their rules.

visibility()          the definition, O(P^2) per pixel: track p is hidden by a track when SOME eligible q != p is drawn there and
                      float32(d_p - d_q) > delta.  Every comparison in float32, as the kernel makes it.
visibility_two_min()  the form the kernel computes, O(P): float32(d_p - m_p) > delta with m_p the smallest eligible drawn depth of a
                      track other than p, from the smallest and second smallest depth and the index of the smallest.
                      tests/test_track_occ_host.py checks that the two agree.
update()              one frame of the state machine with the occluded state.  A track that is not occluded is handed to
                      tests/track_reference.py's update, unchanged: rules 2 to 6 are stated once.
occ_table()           the scripted 12-frame, 7-track table that reaches every branch of the occluded state."""
import numpy as np

import track_reference as R

LOST, REINIT, OCCLUDED = R.LOST, R.REINIT, 16384
OCC_TRACKS, OCC_DEPTH = 1, 2
MODES = {"tracks": OCC_TRACKS, "depth": OCC_DEPTH, "both": OCC_TRACKS | OCC_DEPTH}


def drawn(d):
    """0 < d < +inf; NaN, +inf, 0 and negatives are not drawn"""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return (d > 0) & (d < np.inf)


def _exceeds(a, b, delta):
    """float32(a - b) > delta, elementwise in float32"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float32) > np.float32(delta)


def _hidden_by_depth(depth, depth_frame, mode, delta):
    P = depth.shape[0]
    if not mode & OCC_DEPTH:
        return np.zeros(depth.shape, bool)
    o = np.asarray(depth_frame, np.float32).reshape(depth.shape[1:])
    return np.stack([drawn(o) & _exceeds(depth[p], o, delta) for p in range(P)])


def _finish(depth, dr, by_track, by_depth):
    vis = dr & ~by_track & ~by_depth
    out = np.where(vis, depth, np.float32(0.0)).astype(np.float32)
    counts = np.stack([dr.sum((1, 2)), vis.sum((1, 2)), (dr & by_track).sum((1, 2)), (dr & ~by_track & by_depth).sum((1, 2))], axis=1)
    return out[:, None], counts.astype(np.int32)


def visibility(depth_rendered, depth_frame, occluder_ok, mode, delta):
    """depth_rendered (P,1,H,W) f32, depth_frame (H,W) f32 or None, occluder_ok (P,) or None, mode a key of MODES or its bits
    -> depth_visible (P,1,H,W) f32, counts (P,4) int32 = {drawn, visible, hidden by a track, hidden by the frame's depth only}"""
    mode = MODES.get(mode, mode)
    depth = np.asarray(depth_rendered, np.float32)[:, 0]
    P = depth.shape[0]
    ok = np.ones(P, bool) if occluder_ok is None else np.asarray(occluder_ok) != 0
    dr = drawn(depth)
    by_track = np.zeros(depth.shape, bool)
    if mode & OCC_TRACKS:
        for p in range(P):
            for q in range(P):
                if q != p and ok[q]:
                    by_track[p] |= dr[q] & _exceeds(depth[p], depth[q], delta)
    return _finish(depth, dr, by_track, _hidden_by_depth(depth, depth_frame, mode, delta))


def visibility_two_min(depth_rendered, depth_frame, occluder_ok, mode, delta):
    """the same through the two smallest eligible depths per pixel"""
    mode = MODES.get(mode, mode)
    depth = np.asarray(depth_rendered, np.float32)[:, 0]
    P = depth.shape[0]
    ok = np.ones(P, bool) if occluder_ok is None else np.asarray(occluder_ok) != 0
    dr = drawn(depth)
    m1 = np.full(depth.shape[1:], np.inf, np.float32)
    m2, i1 = m1.copy(), np.full(depth.shape[1:], -1)
    by_track = np.zeros(depth.shape, bool)
    if mode & OCC_TRACKS:
        for p in range(P):
            if not ok[p]:
                continue
            first = dr[p] & (depth[p] < m1)
            second = dr[p] & ~first & (depth[p] < m2)
            m2 = np.where(first, m1, np.where(second, depth[p], m2))
            m1 = np.where(first, depth[p], m1)
            i1 = np.where(first, p, i1)
        for p in range(P):
            by_track[p] = _exceeds(depth[p], np.where(i1 == p, m2, m1), delta)
    return _finish(depth, dr, by_track, _hidden_by_depth(depth, depth_frame, mode, delta))


def boundary_planes(rng, P, H, W, delta):
    """(P,1,H,W) f32 renders and an (H,W) f32 frame depth drawn from the values at which the rules can go wrong: a few base depths
    (ties), base + delta exactly, one float32 step either side of it, far behind, NaN, +inf, 0, -0, negatives, and plain random"""
    delta = np.float32(delta)
    base = np.array([0.5, 0.75, 1.0], np.float32)
    at = (base + delta).astype(np.float32)
    vals = np.concatenate([base, at, np.nextafter(at, np.float32(np.inf)), np.nextafter(at, np.float32(0)), base + np.float32(0.2),
                           np.array([np.nan, np.inf, 0.0, -0.0, -1.0, -np.inf], np.float32)]).astype(np.float32)

    def draw(shape):
        out = vals[rng.randint(0, len(vals), size=shape)]
        rnd = rng.uniform(0.4, 1.3, size=shape).astype(np.float32)
        return np.where(rng.rand(*shape) < 0.25, rnd, out).astype(np.float32)

    return draw((P, 1, H, W)), draw((H, W))


# ------------------------------------------------------------------------------------------------ the state machine
def new_state(P, Wn):
    st = R.new_state(P, Wn)
    st["occ_age"] = np.zeros(P, np.int32)
    return st


def _fatal(status, fatal_mask, pose_new, znear, zfar):
    return (status & fatal_mask) != 0 or not np.all(np.isfinite(pose_new)) or not (znear <= pose_new[2, 3] <= zfar)


def update(state, pose_before, pose_new, status_rows, fatal_mask, score, min_score, reinit_pose, reinit_valid, lost_rot_deg, lost_trans_m,
           znear, zfar, counts, min_visible, max_occluded, pose_pred, coast_pushes_ring=False):
    """one frame, in place on `state` (track_reference's plus occ_age) -> dict(flags, step, mean, visible, pose_track, occluder_ok).
    coast_pushes_ring: a deliberately wrong variant for a negative control (the step of a hidden track enters the ring)"""
    hist, age, ring, ring_n, ring_pos, occ_age = (state[k] for k in ("hist", "age", "ring", "ring_n", "ring_pos", "occ_age"))
    P, Wn = ring.shape[0], ring.shape[1]
    counts = np.asarray(counts).reshape(P, 4)
    status_rows = np.asarray(status_rows).reshape(-1, P)
    flags, step, mean = np.zeros(P, np.int32), np.zeros((P, 2)), np.zeros((P, 2))
    visible, ok = np.zeros(P, np.float32), np.ones(P, np.int32)
    for p in range(P):
        status = 0
        for row in status_rows:
            status |= int(row[p])
        n_drawn, n_seen = int(counts[p, 0]), int(counts[p, 1])
        visible[p] = np.float32(np.float64(n_seen) / np.float64(n_drawn)) if n_drawn > 0 else np.float32(0)
        occluded = (not _fatal(status, fatal_mask, pose_new[p], znear, zfar) and n_drawn > 0
                    and np.float64(n_seen) < np.float64(np.float32(min_visible)) * n_drawn)
        if not occluded:   # rules 2 to 6 as they stand, on this track alone
            sub = {k: state[k][p:p + 1] for k in ("hist", "age", "ring", "ring_n", "ring_pos")}
            f, s, m = R.update(sub, pose_before[p:p + 1], pose_new[p:p + 1], status_rows[:, p:p + 1], fatal_mask,
                               None if score is None else score[p:p + 1], min_score, None if reinit_pose is None else reinit_pose[p:p + 1],
                               None if reinit_valid is None else reinit_valid[p:p + 1], lost_rot_deg, lost_trans_m, znear, zfar)
            flags[p], step[p], mean[p] = f[0], s[0], m[0]
            occ_age[p] = 0
        else:
            Tb, Tn = np.asarray(pose_before[p], np.float64), np.asarray(pose_new[p], np.float64)
            with np.errstate(invalid="ignore"):
                rot = R.angle_deg(Tn[:, :3] @ Tb[:, :3].T)
                trans = float(np.sqrt(np.sum((Tn[:, 3] - Tb[:, 3]) ** 2)))
            step[p] = (rot if np.isfinite(rot) else np.inf, trans if np.isfinite(trans) else np.inf)
            if coast_pushes_ring:
                ring[p, ring_pos[p]] = step[p]
                ring_pos[p] = (ring_pos[p] + 1) % Wn
                ring_n[p] = min(ring_n[p] + 1, Wn)
            n = int(ring_n[p])
            tot = np.zeros(2)
            for k in range(n):   # oldest first
                tot = tot + ring[p, (ring_pos[p] - n + k) % Wn].astype(np.float64)
            mean[p] = tot / n if n else 0.0
            status |= OCCLUDED
            pred = np.asarray(pose_pred[p], np.float32)
            if occ_age[p] < max_occluded and np.all(np.isfinite(pred)) and znear <= pred[2, 3] <= zfar:   # coasts
                hist[p, 0] = hist[p, 1]
                hist[p, 1] = pred
                age[p] = min(age[p] + 1, 2)
                occ_age[p] += 1
            else:
                occ_age[p] = 0
                if reinit_valid is not None and reinit_valid[p] != 0:   # rule 5
                    hist[p, 1] = reinit_pose[p]
                    age[p] = 1
                    ring[p] = 0
                    ring_n[p] = ring_pos[p] = 0
                    status |= LOST | REINIT
                else:                                                   # rule 6
                    age[p] = min(age[p], 1)
                    status |= LOST
            flags[p] = status
        ok[p] = 0 if (flags[p] & LOST) and not (flags[p] & REINIT) else 1
    return dict(flags=flags, step=step, mean=mean, visible=visible, pose_track=hist[:, 1].copy(), occluder_ok=ok)


# ---- the scripted table of the occluded state: track_reference.TABLE's thresholds, min_visible 0.25 (exact in float32), a budget of 2
OCC_TABLE = dict(R.TABLE, frames=12, tracks=7, min_visible=0.25, max_occluded=2)
DRAWN = 100


def occ_table():
    """-> list of 12 frames, each a dict(pose_before, pose_new, pose_pred, reinit_pose (7,3,4) f32, status_rows (2,7), reinit_valid (7,),
    counts (7,4) i32, score (7,) f32).  Every track takes small steps; the state before frame 0 has age 1.  What each track is for:
      0  always wholly visible: never flagged.  Exactly min_visible of it (25 of 100) at frame 6: not occluded (the test is <)
      1  24 of 100 visible at frames 0-3: coasts at age 1, then at age 2, the budget is spent at frame 2 with nothing offered (rule 6,
         OCCLUDED | LOST, occ_age back to 0), so frame 3 coasts again on a fresh budget; visible from frame 4: recovers
      2  hidden at frames 3-5 with a pose offered at frame 5 (OCCLUDED | LOST | REINIT: rule 5); its score is below the bar at frames 3
         and 4, which a coasting track does not look at
      3  hidden at frames 4-5 with a fatal status bit at frame 4: fatal wins (LOST, not OCCLUDED), frame 5 coasts
      4  hidden at frame 2 with a NaN in pose_pred (OCCLUDED | LOST), at frame 7 with pose_pred behind zfar (the same), coasts at 8
      5  nothing drawn at frame 3 (counts 0): not occluded, the plain rules; hidden at frames 6-7 and back at 8: occ_age 0 again, and
         ring_n and ring_pos have not advanced over the gap
      6  hidden at frames 1-2 with large steps before and after (the window rule): the ring is full at frame 4 instead of frame 2"""
    F, P = OCC_TABLE["frames"], OCC_TABLE["tracks"]
    rng = np.random.RandomState(11)
    hidden = {1: (0, 1, 2, 3), 2: (3, 4, 5), 3: (4, 5), 4: (2, 7, 8), 5: (6, 7), 6: (1, 2)}
    frames = []
    for f in range(F):
        before = np.stack([R.pose_of(0.01 * rng.randn(3) + [0.3 * p, 0.1, -0.2], [0.01 * p, -0.02, 0.8 + 0.05 * p]) for p in range(P)])
        new = before.copy()
        for p in range(P):
            w = rng.randn(3)
            w *= np.radians(8.0 if p == 6 else 1.0) / np.linalg.norm(w)
            new[p, :, :3] = (R.so3_exp(w) @ before[p, :, :3].astype(np.float64)).astype(np.float32)
            new[p, :, 3] += np.float32(0.004) * np.array([0.6, 0.0, 0.8], np.float32)
        pred = np.stack([R.pose_of(0.02 * rng.randn(3) + [0.3 * p, 0.1, -0.2], [0.01 * p, 0.03, 0.7 + 0.05 * p]) for p in range(P)])
        offered = np.stack([R.pose_of(0.02 * rng.randn(3) + [0.1, 0.2 * p, 0.0], [0.0, 0.01 * p, 0.9]) for p in range(P)])
        status = np.zeros((2, P), np.int32)
        score = np.full(P, 0.9, np.float32)
        valid = np.zeros(P, np.int32)
        counts = np.tile(np.array([DRAWN, DRAWN, 0, 0], np.int32), (P, 1))
        for p, at in hidden.items():
            if f in at:
                counts[p] = (DRAWN, 24, 50, 26)
        if f == 6:
            counts[0] = (DRAWN, 25, 75, 0)
        if f in (3, 4):
            score[2] = 0.1
        if f == 5:
            valid[2] = 1
        if f == 4:
            status[1, 3] = R.REN_BOX_EMPTY
        if f == 2:
            pred[4, 1, 1] = np.nan
        if f == 7:
            pred[4, 2, 3] = 6.5
        if f == 3:
            counts[5] = 0
        frames.append(dict(pose_before=before, pose_new=new, pose_pred=pred, reinit_pose=offered, status_rows=status, reinit_valid=valid,
                           counts=counts, score=score))
    return frames


# frames at which each track carries each flag in occ_table() (asserted by the host test against update())
EXPECT_OCCLUDED = {0: [], 1: [0, 1, 2, 3], 2: [3, 4, 5], 3: [5], 4: [2, 7, 8], 5: [6, 7], 6: [1, 2]}
EXPECT_LOST = {0: [], 1: [2], 2: [5], 3: [4], 4: [2, 7], 5: [], 6: [4, 5, 6, 7, 8, 9, 10, 11]}
EXPECT_REINIT = {0: [], 1: [], 2: [5], 3: [], 4: [], 5: [], 6: []}


def table_state(frames, T=OCC_TABLE):
    st = new_state(T["tracks"], T["Wn"])
    st["hist"][:, 1] = frames[0]["pose_before"]
    st["hist"][:, 0] = frames[0]["pose_before"]
    st["age"][:] = 1
    return st


def run_table(frames, T=OCC_TABLE, min_visible=None, **variant):
    """the reference over a table from the fresh state -> per frame (outputs dict, copy of the state after the frame).  Frames
    without counts / pose_pred (track_reference.scripted_table()) get wholly visible counts and pose_before as the prediction"""
    st = table_state(frames, T)
    P = T["tracks"]
    out = []
    for fr in frames:
        counts = fr.get("counts", np.tile(np.array([DRAWN, DRAWN, 0, 0], np.int32), (P, 1)))
        o = update(st, fr["pose_before"], fr["pose_new"], fr["status_rows"], T["fatal_mask"], fr["score"], T["min_score"], fr["reinit_pose"],
                   fr["reinit_valid"], T["lost_rot_deg"], T["lost_trans_m"], T["znear"], T["zfar"], counts,
                   T.get("min_visible", 0.0) if min_visible is None else min_visible, T.get("max_occluded", 0), fr.get("pose_pred", fr["pose_before"]),
                   **variant)
        out.append((o, {k: v.copy() for k, v in st.items()}))
    return out
