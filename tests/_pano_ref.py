"""numpy restatement of the stereo panorama stage, written from the reference's lines (examples/stereo_panorama_tools.cpp), and the scenes its tests share.

plan():        :496-616 in float64 -- the theta / phi grids, the three signed angles and their tests, alpha, colout, and `ok` by the all-rows rule of
               get_synthetic_column_maps (:69-106); the owner of an output column is the ok job of the highest pair index (the reference overwrites with copyTo).
               It also returns the smallest distance of any decision from its threshold, so that a test can assert that no case hangs on a last bit.
synthesize():  the pixel path on numpy float64 / float32 arrays in exactly the operation order of include/ssfm.h and csrc/pano_host.h.  numpy never fuses a
               multiply-add; every operation is one correctly rounded IEEE operation, like the kernel's.
Poses are row-major, x_cam = R x_world + t."""
import numpy as np

F32 = np.float32
LIMIT = F32(2.0 ** 30)


def so3exp(r):
    r = np.asarray(r, np.float64); th = np.sqrt(r @ r)
    if th < 1e-10:
        return np.eye(3)
    v = r / th
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + np.sin(th) * K + ((1 - np.cos(th)) * K) @ K


def _signed_angle(a, b, up):
    return np.arctan2(np.cross(a, b) @ up, (a * b).sum(-1))


def _project(v, up):
    return v - up * (v @ up)[..., None]


def phis(num_phi, step_deg=1.0):
    if num_phi == 1:
        return np.zeros(1)
    lo = (-(num_phi - 1) / 2.) * step_deg * np.pi / 180.; hi = ((num_phi - 1) / 2.) * step_deg * np.pi / 180.
    return np.array([lo + i * (hi - lo) / (num_phi - 1) for i in range(num_phi)])


def row_map(tan_phi, sR, R, t, focal, cx, cy, height, depth=10.0, radius=0.5, factor=1.2):
    """tan_phi [m], sR [m, 3, 3], R [m, 3, 3], t [m, 3] -> x, y, z [m, height] in float64: the order of csrc/pano_host.h"""
    y = np.arange(height, dtype=np.float64)[None, :]
    sy = (y - cy) / (focal * factor); d1 = sy * depth
    d0 = (tan_phi * depth)[:, None]; d2 = 1.0 * depth + radius
    w = [(sR[:, 0, i, None] * d0 + sR[:, 1, i, None] * d1) + sR[:, 2, i, None] * d2 for i in range(3)]
    X = [((R[:, i, 0, None] * w[0] + R[:, i, 1, None] * w[1]) + R[:, i, 2, None] * w[2]) + t[:, i, None] for i in range(3)]
    with np.errstate(all="ignore"):
        return (focal * X[0]) / X[2] + cx, (focal * X[1]) / X[2] + cy, X[2]


def plan(R, t, intrinsics, height, pano_width, num_phi=9, phi_step_deg=1.0, depth=10.0, synth_radius=0.5, synth_focal_factor=1.2, is_loop=1, **_):
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3); n = len(R)
    focal, cx, cy = intrinsics
    up = np.array([0., 1., 0.]); synth_t = np.array([0., 0., -synth_radius])
    theta_step = (np.pi - (-np.pi)) / (pano_width - 1)
    thetas = np.array([-np.pi + i * theta_step for i in range(pano_width)])
    ph = phis(num_phi, phi_step_deg); tan_phi = np.tan(ph)
    shift = np.array([int(np.floor(abs(p / theta_step) + 0.5)) * (1 if p >= 0 else -1) for p in ph])           # C's round(): halves away from zero
    margin = min([np.inf] + [abs(abs(p / theta_step) % 1.0 - 0.5) for p in ph])
    sR = np.stack([so3exp([0, -th, 0]) for th in thetas])                                                         # [T, 3, 3]
    C_D = -np.einsum("tji,j->ti", sR, synth_t)
    r_D = np.einsum("tji,pj->tpi", sR, np.stack([tan_phi, np.zeros(num_phi), np.ones(num_phi)], 1) - synth_t)     # [T, P, 3]
    rs_D = _project(r_D, up)
    out = {k: [] for k in ("pair", "theta", "phi", "col", "alpha")}
    pairs = 0 if n == 0 else (n if is_loop else n - 1)
    for k in range(pairs):
        l, r = k, (k + 1) % n
        C_L = -R[l].T @ t[l]; C_R = -R[r].T @ t[r]
        rs_L = _project(C_L - C_D, up); rs_R = _project(C_R - C_D, up)                                            # [T, 3]
        a_LD = _signed_angle(rs_L[:, None, :], rs_D, up); a_RD = _signed_angle(rs_R[:, None, :], rs_D, up); a_LR = _signed_angle(rs_L, rs_R, up)[:, None]
        margin = min(margin, np.abs(a_LD * a_RD).min(), np.abs(np.abs(a_LD) - np.pi / 2).min(), np.abs(np.abs(a_RD) - np.pi / 2).min())
        keep = (a_LD * a_RD < 0) & ~(np.abs(a_LD) >= np.pi / 2) & ~(np.abs(a_RD) >= np.pi / 2)
        th, p = np.nonzero(keep)                                                                                  # theta-major, then phi: the reference's order
        with np.errstate(all="ignore"):
            alpha = (np.abs(a_LD) / np.abs(a_LR))[th, p]
        out["pair"].append(np.full(len(th), k)); out["theta"].append(th); out["phi"].append(p); out["alpha"].append(alpha)
        out["col"].append(np.mod(th + shift[p], pano_width))
    P = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in out.items()}
    for k in ("pair", "theta", "phi", "col"):
        P[k] = P[k].astype(np.int32)
    m = len(P["pair"])
    P["tan_phi"] = tan_phi[P["phi"]] if m else np.zeros(0); P["synth_R"] = sR[P["theta"]] if m else np.zeros((0, 3, 3))
    ok = np.zeros(m, np.uint8)
    if m:
        l = P["pair"]; r = (l + 1) % n
        zL = row_map(P["tan_phi"], P["synth_R"], R[l], t[l], focal, cx, cy, height, depth, synth_radius, synth_focal_factor)[2]
        zR = row_map(P["tan_phi"], P["synth_R"], R[r], t[r], focal, cx, cy, height, depth, synth_radius, synth_focal_factor)[2]
        ok = ((zL > 0).all(1) & (zR > 0).all(1)).astype(np.uint8)
        margin = min(margin, np.abs(zL).min(), np.abs(zR).min())
    P["ok"] = ok
    owner = np.full((num_phi, pano_width), -1, np.int32); owner_job = np.full((num_phi, pano_width), -1, np.int64); overwrites = 0
    for j in range(m):
        if ok[j]:
            overwrites += owner[P["phi"][j], P["col"][j]] >= 0
            owner[P["phi"][j], P["col"][j]] = P["pair"][j]; owner_job[P["phi"][j], P["col"][j]] = j
    P["owner"] = owner; P["owner_job"] = owner_job; P["overwrites"] = int(overwrites); P["margin"] = float(margin)
    return P


def owner_jobs(P, num_phi, pano_width):
    """index of the owning job of every output column from the job table alone (a library plan has no owner_job): the ok job of the highest pair"""
    oj = np.full((num_phi, pano_width), -1, np.int64)
    for j in range(len(P["pair"])):
        if P["ok"][j]:
            oj[P["phi"][j], P["col"][j]] = j
    return oj


def bilinear(img, x, y, snap, stats=None):
    """img [m, H, W, C] float32 (one image per column job), x, y [m, rows] float32 -> [m, rows, C] float32"""
    m, H, W, _ = img.shape
    with np.errstate(all="ignore"):
        ok = (np.abs(x) <= LIMIT) & (np.abs(y) <= LIMIT)
        if stats is not None:
            stats["invalid"] = stats.get("invalid", 0) + int((~ok).sum())
        x = np.where(ok, x, F32(0)); y = np.where(ok, y, F32(0))
        if snap:
            x = np.rint(x * F32(32)) / F32(32); y = np.rint(y * F32(32)) / F32(32)
        x0 = np.floor(x); y0 = np.floor(y); fx = x - x0; fy = y - y0
        assert x.dtype == F32 and fx.dtype == F32
        ix = x0.astype(np.int64); iy = y0.astype(np.int64)
        one = F32(1)
        w = [(one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx]
        idx = np.arange(m)[:, None]
        taps = []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            inside = ok & (ix + dx >= 0) & (ix + dx < W) & (iy + dy >= 0) & (iy + dy < H)
            v = img[idx, np.clip(iy + dy, 0, H - 1), np.clip(ix + dx, 0, W - 1)]
            taps.append(np.where(inside[..., None], v, F32(0)))
            if stats is not None:
                stats["inside"] = stats.get("inside", 0) + int(inside.sum()); stats["outside"] = stats.get("outside", 0) + int((~inside).sum())
        val = ((taps[0] * w[0][..., None] + taps[1] * w[1][..., None]) + taps[2] * w[2][..., None]) + taps[3] * w[3][..., None]
        assert val.dtype == F32
        return np.where(ok[..., None], val, F32(0))


def to_byte(v):
    with np.errstate(all="ignore"):
        r = np.rint(v)
        return np.where(~(r > 0), F32(0), np.where(r > 255, F32(255), r)).astype(np.uint8)


def synthesize(P, R, t, intrinsics, frames, flows, pano_width, num_phi=9, subpixel_bits=0, depth=10.0, synth_radius=0.5, synth_focal_factor=1.2, stats=None, **_):
    """P: a job table (pair, phi, col, ok, alpha, tan_phi, synth_R) -- the library's own plan in the GPU tests.  -> (panoramas, owner)"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3); t = np.asarray(t, np.float64).reshape(-1, 3); n = len(R)
    focal, cx, cy = intrinsics
    frames = np.asarray(frames); H, W = frames.shape[1:3]
    out = np.zeros((num_phi, H, pano_width, 3), np.uint8)
    oj = owner_jobs(P, num_phi, pano_width)
    owner = np.where(oj >= 0, P["pair"][np.maximum(oj, 0)] if len(P["pair"]) else -1, -1).astype(np.int32)
    pp, cc = np.nonzero(oj >= 0)
    if len(pp) == 0:
        return out, owner
    j = oj[pp, cc]; l = P["pair"][j]; r = (l + 1) % n
    args = (focal, cx, cy, H, depth, synth_radius, synth_focal_factor)
    xL, yL, _ = row_map(P["tan_phi"][j], P["synth_R"][j], R[l], t[l], *args); xR, yR, _ = row_map(P["tan_phi"][j], P["synth_R"][j], R[r], t[r], *args)
    xL, yL, xR, yR = (a.astype(F32) for a in (xL, yL, xR, yR))
    alpha = P["alpha"][j]
    with np.errstate(all="ignore"):
        a1 = alpha.astype(F32)[:, None]; a0 = (1.0 - alpha).astype(F32)[:, None]
        snap = subpixel_bits == 5
        sLx, sLy, sRx, sRy = xL, yL, xR, yR
        if flows is not None:
            fwd = np.stack([np.asarray(flows[0][k], F32) for k in l]); bwd = np.stack([np.asarray(flows[1][k], F32) for k in l])
            F_LR = bilinear(fwd, xL, yL, snap); F_RL = bilinear(bwd, xR, yR, snap)
            Fs_LRx = (xR - xL) - F_LR[..., 0]; Fs_LRy = (yR - yL) - F_LR[..., 1]; Fs_RLx = (xL - xR) - F_RL[..., 0]; Fs_RLy = (yL - yR) - F_RL[..., 1]
            sLx = xL * F32(1) + Fs_LRx * a1; sLy = yL * F32(1) + Fs_LRy * a1
            sRx = xR * F32(1) + Fs_RLx * a0; sRy = yR * F32(1) + Fs_RLy * a0
        ff = frames.astype(F32)
        I_L = bilinear(ff[l], sLx, sLy, snap, stats); I_R = bilinear(ff[r], sRx, sRy, snap, stats)
        res = I_L * a0[..., None] + I_R * a1[..., None]
        assert res.dtype == F32
    out[pp, :, cc, :] = to_byte(res)
    return out, owner


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------------

def circle_poses(n, rng, t_noise=0.02, yaw_jitter=0.3, tilt_sigma=0.05):
    """n cameras looking outward from the unit circle: t ~ (0, 0, -1), yaw = k * spacing with jitter, a small random tilt about x and z"""
    R, t = [], []
    for k in range(n):
        a = (k + rng.uniform(-yaw_jitter, yaw_jitter)) * 2 * np.pi / n
        c, s = np.cos(a), np.sin(a)
        yaw = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        tilt = so3exp([rng.normal(0, tilt_sigma), 0, rng.normal(0, tilt_sigma)])
        R.append(tilt @ yaw); t.append(np.array([0, 0, -1.0]) + rng.normal(0, t_noise, 3))
    return np.array(R), np.array(t)


def reorient(R, t, k, extra):
    """camera k turned about its own centre by the rotation `extra` (applied in the camera frame)"""
    R = R.copy(); t = t.copy()
    c = -R[k].T @ t[k]
    R[k] = extra @ R[k]; t[k] = -R[k] @ c
    return R, t


def scene1(seed=1):
    rng = np.random.default_rng(seed)
    R, t = circle_poses(7, rng)
    return dict(R=R, t=t, intr=(40.0, 24.0, 18.5), width=48, height=37, pano_width=193)


def scene2(seed=17):
    rng = np.random.default_rng(seed)
    R, t = circle_poses(12, rng, tilt_sigma=0.6)
    return dict(R=R, t=t, intr=(40.0, 24.0, 18.5), width=48, height=37, pano_width=130)


def scene3(kind="yaw", seed=1):
    s = scene1(seed)
    if kind == "yaw":
        s["R"], s["t"] = reorient(s["R"], s["t"], 3, so3exp([0, 1.7, 0]))
    else:
        s["R"], s["t"] = reorient(s["R"], s["t"], 3, so3exp([1.1, 0, 0])); s["intr"] = (12.0, 24.0, 18.5)
    return s


def texture(n, height, width, seed):
    """smooth random textures: a few low-frequency waves per channel plus a little noise, full byte range"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    out = np.zeros((n, height, width, 3))
    for f in range(n):
        for c in range(3):
            a, b, p, q = rng.uniform(0.05, 0.5, 4)
            out[f, :, :, c] = 127.5 + 90 * np.sin(a * x + b * y + rng.uniform(0, 6)) * np.cos(p * x - q * y + rng.uniform(0, 6)) + rng.normal(0, 12, (height, width))
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def smooth_flows(n, height, width, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    def field():
        out = np.zeros((n, height, width, 2), np.float32)
        for f in range(n):
            for c in range(2):
                a, b = rng.uniform(0.05, 0.3, 2)
                out[f, :, :, c] = scale * np.sin(a * x + rng.uniform(0, 6)) * np.cos(b * y + rng.uniform(0, 6)) + rng.normal(0, 0.05 * scale, (height, width))
        return out
    return field(), field()
