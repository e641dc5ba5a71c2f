"""Plain numpy float64 restatement of dim_track_predict and dim_track_update (include/deepim_hip.h), written from their rules.

State of P tracks: hist (P,2,3,4) with [1] the last accepted pose and [0] the one before, age (P,) in {0,1,2}, ring (P,Wn,2) of
(rotation step in degrees, translation step in metres), ring_n, ring_pos (P,).  `scripted_table()` is the 14-frame, 6-track script that
reaches every branch of the update; tests/test_track_host.py asserts what it flags and tests/test_gpu_track_kernels.py runs it on
the device."""
import numpy as np

LOST, REINIT = 4096, 8192
REN_BOX_EMPTY = 2


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_exp(w):
    """Rodrigues: exp(hat(w))"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3) + hat(w)
    K = hat(w / th)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def sin_cos(D):
    """-> (v, s, c): v = sin(angle) * axis from the antisymmetric part, s = |v|, c = (tr D - 1) / 2"""
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return v, float(np.linalg.norm(v)), 0.5 * (np.trace(D) - 1.0)


def so3_log(D):
    """axis-angle vector of a rotation matrix, stable at 0 and up to pi: the angle is atan2(|v|, c); for c >= -0.5 the axis is v / |v|
    (log = v below |v| = 1e-8), else it is the eigenvector of the symmetric part: (D + D^T) / 2 = c I + (1 - c) a a^T"""
    D = np.asarray(D, np.float64)
    v, s, c = sin_cos(D)
    angle = np.arctan2(s, c)
    if c >= -0.5:
        return v.copy() if s < 1e-8 else angle * v / s
    M = (0.5 * (D + D.T) - c * np.eye(3)) / (1.0 - c)
    k = int(np.argmax(np.diag(M)))
    a = M[k] / np.sqrt(M[k, k])
    a = a / np.linalg.norm(a)
    if a @ v < 0:
        a = -a
    return angle * a


def angle_deg(D):
    _, s, c = sin_cos(np.asarray(D, np.float64))
    return float(np.degrees(np.arctan2(s, c)))


def predict(hist, age, mode, alpha):
    """-> (P,3,4) float64 and hold (P,) bool: where hold is set the row is hist[1] itself (the kernel copies its bits)"""
    hist = np.asarray(hist)
    P = hist.shape[0]
    out = np.array(hist[:, 1], dtype=np.float64)
    hold = np.ones(P, dtype=bool)
    for p in range(P):
        prev, last = hist[p, 0].astype(np.float64), hist[p, 1].astype(np.float64)
        if mode != "velocity" or age[p] < 2 or not np.all(np.isfinite(hist[p])) or not prev[2, 3] > 0 or not last[2, 3] > 0:
            continue
        hold[p] = False
        w = so3_log(last[:, :3] @ prev[:, :3].T)
        R = so3_exp(alpha * w) @ last[:, :3]
        zp, zl = prev[2, 3], last[2, 3]
        up, vp, ul, vl = prev[0, 3] / zp, prev[1, 3] / zp, last[0, 3] / zl, last[1, 3] / zl
        z = zl * (zl / zp) ** alpha
        u, v = ul + alpha * (ul - up), vl + alpha * (vl - vp)
        out[p, :, :3] = R
        out[p, :, 3] = (u * z, v * z, z)
    return out, hold


def new_state(P, Wn):
    return dict(hist=np.zeros((P, 2, 3, 4), np.float32), age=np.zeros(P, np.int32), ring=np.zeros((P, Wn, 2), np.float32),
                ring_n=np.zeros(P, np.int32), ring_pos=np.zeros(P, np.int32))


def update(state, pose_before, pose_new, status_rows, fatal_mask, score, min_score, reinit_pose, reinit_valid, lost_rot_deg, lost_trans_m,
           znear, zfar, swap_5_6=False, window_on_part_full=False):
    """one frame of the state machine, in place on `state` -> flags (P,) int32, step (P,2), mean (P,2) float64.
    swap_5_6 / window_on_part_full: deliberately wrong variants for negative controls (a lost track with an offered pose takes rule
    6; the window rule acts on a ring that is not full yet)"""
    hist, age, ring, ring_n, ring_pos = (state[k] for k in ("hist", "age", "ring", "ring_n", "ring_pos"))
    P, Wn = ring.shape[0], ring.shape[1]
    flags, step, mean = np.zeros(P, np.int32), np.zeros((P, 2)), np.zeros((P, 2))
    for p in range(P):
        Tb, Tn = np.asarray(pose_before[p], np.float64), np.asarray(pose_new[p], np.float64)
        status = 0
        for row in np.asarray(status_rows).reshape(-1, P):
            status |= int(row[p])
        with np.errstate(invalid="ignore"):
            rot = angle_deg(Tn[:, :3] @ Tb[:, :3].T)
            trans = float(np.sqrt(np.sum((Tn[:, 3] - Tb[:, 3]) ** 2)))
        rot = rot if np.isfinite(rot) else np.inf
        trans = trans if np.isfinite(trans) else np.inf
        step[p] = (rot, trans)
        ring[p, ring_pos[p]] = (rot, trans)
        ring_pos[p] = (ring_pos[p] + 1) % Wn
        ring_n[p] = min(ring_n[p] + 1, Wn)
        n = int(ring_n[p])
        tot = np.zeros(2)
        for k in range(n):   # oldest first
            tot = tot + ring[p, (ring_pos[p] - n + k) % Wn].astype(np.float64)
        mean[p] = tot / n
        lost = (status & fatal_mask) != 0 or not np.all(np.isfinite(pose_new[p]))
        lost = lost or not (znear <= pose_new[p][2, 3] <= zfar)
        if score is not None:
            lost = lost or not (score[p] >= min_score)
        if n == Wn or window_on_part_full:
            lost = lost or mean[p, 0] > lost_rot_deg or mean[p, 1] > lost_trans_m
        offered = reinit_valid is not None and reinit_valid[p] != 0
        if swap_5_6:
            offered = False
        if not lost:
            hist[p, 0] = hist[p, 1]
            hist[p, 1] = pose_new[p]
            age[p] = min(age[p] + 1, 2)
        elif offered:
            hist[p, 1] = reinit_pose[p]
            age[p] = 1
            ring[p] = 0
            ring_n[p] = ring_pos[p] = 0
            status |= LOST | REINIT
        else:
            age[p] = min(age[p], 1)
            status |= LOST
        flags[p] = status
    return flags, step, mean


# ---- poses for the tests

def pose_of(w, t):
    """(3,4) float32: rotation exp(hat(w)), translation t"""
    return np.concatenate([so3_exp(np.asarray(w, np.float64)), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(np.float32)


def constant_velocity_poses(n, R0, w, uv0, duv, z0, zr):
    """n float64 poses: R_k = exp(k hat(w)) R0 (constant angular velocity in the camera frame), (u, v) = uv0 + k duv, z = z0 zr^k --
    the trajectories on which the velocity predictor with alpha = 1 is exact"""
    out = np.zeros((n, 3, 4))
    for k in range(n):
        z = z0 * zr ** k
        u, v = uv0[0] + k * duv[0], uv0[1] + k * duv[1]
        out[k, :, :3] = so3_exp(k * np.asarray(w, np.float64)) @ R0
        out[k, :, 3] = (u * z, v * z, z)
    return out


# ---- the scripted table: Wn = 3, lost_rot_deg = 5, lost_trans_m = 0.05, znear 0.25, zfar 6, fatal_mask = REN_BOX_EMPTY, min_score 0.5
TABLE = dict(Wn=3, lost_rot_deg=5.0, lost_trans_m=0.05, znear=0.25, zfar=6.0, fatal_mask=REN_BOX_EMPTY, min_score=0.5, frames=14, tracks=6)


def scripted_table():
    """-> list of 14 frames, each a dict(pose_before, pose_new (6,3,4) f32, status_rows (2,6) i32, score (6,) f32, reinit_pose (6,3,4) f32,
    reinit_valid (6,) i32).  What each track is for:
      0  small steps throughout: never lost (rule 4 only; the ring wraps)
      1  a fatal status bit at frame 2 without an offered pose (rule 6), fine again afterwards; a NaN pose at frame 9 with one (rule 5)
      2  t_z behind zfar at frame 4, offered (rule 5); score below the bar at frame 8, not offered (rule 6); a NaN score at frame 11 (rule 6)
      3  large steps from frame 0: the window rule bites at frame 2, when the ring is full and not before, offered (rule 5); the grace of the
         emptied ring: lost again at frame 5 only
      4  a non-finite pose_before at frame 3: the step is +inf and stays in the ring (full since frame 2) for three frames, so the window
         rule loses the track at frames 3, 4 and 5 -- not offered (rule 6: the ring is kept) -- until the +inf is overwritten at frame 6
      5  large translation steps with the window rule, not offered: lost from frame 2 on, every frame (rule 6, the ring is kept)"""
    F, P = TABLE["frames"], TABLE["tracks"]
    rng = np.random.RandomState(5)
    frames = []
    for f in range(F):
        before = np.stack([pose_of(0.01 * rng.randn(3) + [0.3 * p, 0.1, -0.2], [0.01 * p, -0.02, 0.8 + 0.05 * p]) for p in range(P)])
        new = before.copy()
        for p in range(P):
            big_rot = p == 3
            big_trans = p == 5
            w = rng.randn(3)
            w *= np.radians(8.0 if big_rot else 1.0) / np.linalg.norm(w)
            new[p, :, :3] = (so3_exp(w) @ before[p, :, :3].astype(np.float64)).astype(np.float32)
            new[p, :, 3] += np.float32(0.08 if big_trans else 0.004) * np.array([0.6, 0.0, 0.8], np.float32)
        status = np.zeros((2, P), np.int32)
        status[0, 0] = 32          # a bit outside fatal_mask never loses a track
        score = np.full(P, 0.9, np.float32)
        valid = np.zeros(P, np.int32)
        if f == 2:
            status[1, 1] = REN_BOX_EMPTY
        if f == 9:
            new[1, 1, 2] = np.nan
            valid[1] = 1
        if f == 4:
            new[2, 2, 3] = 7.0
            valid[2] = 1
        if f == 8:
            score[2] = 0.3
        if f == 11:
            score[2] = np.nan
        valid[3] = 1
        if f == 3:
            before[4, 0, 3] = np.inf
        offered = np.stack([pose_of(0.02 * rng.randn(3) + [0.1, 0.2 * p, 0.0], [0.0, 0.01 * p, 0.9]) for p in range(P)])
        frames.append(dict(pose_before=before, pose_new=new, status_rows=status, score=score, reinit_pose=offered, reinit_valid=valid))
    return frames


# frames at which each track flags LOST / REINIT in the scripted table (asserted by the host test against update())
EXPECT_LOST = {0: [], 1: [2, 9], 2: [4, 8, 11], 3: [2, 5, 8, 11], 4: [3, 4, 5], 5: list(range(2, 14))}
EXPECT_REINIT = {0: [], 1: [9], 2: [4], 3: [2, 5, 8, 11], 4: [], 5: []}


def run_table(frames, **variant):
    """the reference over the whole table from a fresh state (hist[1] = the first frame's pose_before, age 1) -> per frame
    (flags, step, mean, copy of the state after the frame)"""
    st = new_state(TABLE["tracks"], TABLE["Wn"])
    st["hist"][:, 1] = frames[0]["pose_before"]
    st["hist"][:, 0] = frames[0]["pose_before"]
    st["age"][:] = 1
    out = []
    for fr in frames:
        flags, step, mean = update(st, fr["pose_before"], fr["pose_new"], fr["status_rows"], TABLE["fatal_mask"], fr["score"], TABLE["min_score"],
                                   fr["reinit_pose"], fr["reinit_valid"], TABLE["lost_rot_deg"], TABLE["lost_trans_m"], TABLE["znear"],
                                   TABLE["zfar"], **variant)
        out.append((flags, step, mean, {k: v.copy() for k, v in st.items()}))
    return out
