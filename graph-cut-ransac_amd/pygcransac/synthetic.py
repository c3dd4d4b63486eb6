"""Synthetic rectification problems (inputs M1 / M2).

The reference's example notebook and its SIFT features are not in the snapshot
(``.MISSING_LARGE_BLOBS:1``) and cv2 is absent, so benchmarks and tests use
seeded synthetic features with a known rectifying homography instead.

Feature conventions follow ``examples/utils.py:5-49`` of the reference:
scale features are rows ``(x, y, size)``, orientation features rows
``(x, y, angle_rad)``.  Ground truth uses the reference's own model maths
(``model.h:122-204``): an inlier scale feature satisfies
``alpha^3 * s * (1 - h7 x - h8 y)^-3 = exp(eps)``; an inlier orientation
feature rectifies (``rectifiedAngle``) to ``phi`` or ``phi + pi/2`` plus noise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

WIDTH, HEIGHT = 1368.0, 1824.0          # examples/img/tiled_floor_001.jpg
DEFAULT_SEED = 20251121


@dataclass
class GroundTruth:
    h7: float = 2.0e-4
    h8: float = -1.5e-4
    alpha: float = 0.5
    phi: float = 0.35


def _unrectified_angle(h7, h8, x, y, angle):
    # model.h:167-174 (glibc cos/sin/atan2 via Python's math module)
    ct, st = math.cos(angle), math.sin(angle)
    numer = (x * st - y * ct) * h7 + st
    denom = (-x * st + y * ct) * h8 + ct
    a = math.fmod(math.atan2(numer, denom), 2.0 * math.pi)
    return a + 2.0 * math.pi if a < 0.0 else a


def scale_features(n: int, outlier_ratio: float = 0.5, seed: int = DEFAULT_SEED,
                   gt: GroundTruth = GroundTruth(), noise: float = 0.02, width: float = WIDTH,
                   height: float = HEIGHT):
    """M1: n scale features (x, y, s); returns (features[n,3], inlier_mask)."""
    rng = np.random.default_rng(seed)
    n_out = int(round(n * outlier_ratio))
    n_in = n - n_out
    x = rng.uniform(0.0, width, n)
    y = rng.uniform(0.0, height, n)
    t = 1.0 - gt.h7 * x[:n_in] - gt.h8 * y[:n_in]
    s_in = (t / gt.alpha) ** 3 * np.exp(rng.normal(0.0, noise, n_in))
    s_out = np.exp(rng.uniform(math.log(2.0), math.log(64.0), n_out))
    s = np.concatenate([s_in, s_out])
    truth = np.zeros(n, dtype=bool)
    truth[:n_in] = True
    perm = rng.permutation(n)
    feats = np.stack([x, y, s], axis=1)[perm]
    return np.ascontiguousarray(feats), truth[perm]


def orientation_features(n: int, outlier_ratio: float = 0.5, seed: int = DEFAULT_SEED + 1,
                         gt: GroundTruth = GroundTruth(), noise_deg: float = 0.5, width: float = WIDTH,
                         height: float = HEIGHT):
    """M2 orientation part: n features (x, y, angle); returns (features, inlier_mask)."""
    rng = np.random.default_rng(seed)
    n_out = int(round(n * outlier_ratio))
    n_in = n - n_out
    x = rng.uniform(0.0, width, n)
    y = rng.uniform(0.0, height, n)
    theta = np.empty(n)
    which = rng.integers(0, 2, n_in)
    noise = np.deg2rad(rng.normal(0.0, noise_deg, n_in))
    for i in range(n_in):
        w = 1.0 - gt.h7 * x[i] - gt.h8 * y[i]          # rectifyPoint
        u, v = x[i] / w, y[i] / w
        tr = gt.phi + (math.pi / 2.0) * which[i] + noise[i]
        theta[i] = _unrectified_angle(gt.h7, gt.h8, u, v, tr)
    theta[n_in:] = rng.uniform(0.0, 2.0 * math.pi, n_out)
    truth = np.zeros(n, dtype=bool)
    truth[:n_in] = True
    perm = rng.permutation(n)
    feats = np.stack([x, y, theta], axis=1)[perm]
    return np.ascontiguousarray(feats), truth[perm]


def problem_m1(n: int = 10_000, outlier_ratio: float = 0.5, seed: int = DEFAULT_SEED):
    """Scale-only problem (3-SIFT): features, truth mask, thresholds."""
    f, t = scale_features(n, outlier_ratio, seed)
    return f, t, 0.05


def problem_m2(n_scale: int = 5_000, n_orient: int = 5_000, outlier_ratio: float = 0.5,
               seed: int = DEFAULT_SEED):
    """Hybrid problem (2+2 SIFT): scale feats, orientation feats, truths, thresholds."""
    fs, ts = scale_features(n_scale, outlier_ratio, seed)
    fo, to = orientation_features(n_orient, outlier_ratio, seed + 1)
    return fs, fo, ts, to, 0.05, math.radians(1.0)


# ------------------------------------------------------------ homography ----
# BASELINE configs[2]: N = 5 000 correspondences, 50 % outliers.  Two views of
# a plane: inliers are image-1 points mapped by a ground-truth homography plus
# Gaussian pixel noise; outliers are independent uniform pairs.
H_GT = np.array([[0.92, -0.08, 35.0],
                 [0.06, 0.97, -18.0],
                 [4.0e-5, -3.0e-5, 1.0]])
IMG_W, IMG_H = 1280.0, 960.0


def problem_h(n: int = 5_000, outlier_ratio: float = 0.5, seed: int = DEFAULT_SEED, noise: float = 0.5,
              H: np.ndarray = H_GT):
    """Homography problem: correspondences (n, 4) = (x1, y1, x2, y2), inlier
    truth mask, ground-truth H and the inlier threshold (px)."""
    rng = np.random.default_rng(seed)
    n_out = int(round(n * outlier_ratio))
    n_in = n - n_out
    x1 = rng.uniform(0, IMG_W, n_in)
    y1 = rng.uniform(0, IMG_H, n_in)
    w = H[2, 0] * x1 + H[2, 1] * y1 + H[2, 2]
    x2 = (H[0, 0] * x1 + H[0, 1] * y1 + H[0, 2]) / w + rng.normal(0, noise, n_in)
    y2 = (H[1, 0] * x1 + H[1, 1] * y1 + H[1, 2]) / w + rng.normal(0, noise, n_in)
    inl = np.stack([x1, y1, x2, y2], axis=1)
    out = np.stack([rng.uniform(0, IMG_W, n_out), rng.uniform(0, IMG_H, n_out),
                    rng.uniform(0, IMG_W, n_out), rng.uniform(0, IMG_H, n_out)], axis=1)
    corr = np.concatenate([inl, out])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(n)
    return np.ascontiguousarray(corr[perm]), truth[perm], H.copy(), 2.0


def problem_h_local(n: int = 5_000, outlier_ratio: float = 0.9, seed: int = DEFAULT_SEED, region: float = 0.25,
                    noise: float = 0.5, H: np.ndarray = H_GT):
    """problem_h with the inliers a local structure: their image-1 points lie
    in a seeded `region` x `region` window of the image (fractions of its
    width and height); the outliers stay uniform in both images.  The case
    NAPSAC sampling (csrc/napsac.h) is for."""
    rng = np.random.default_rng(seed)
    n_out = int(round(n * outlier_ratio))
    n_in = n - n_out
    x0 = rng.uniform(0, IMG_W * (1.0 - region))
    y0 = rng.uniform(0, IMG_H * (1.0 - region))
    x1 = rng.uniform(x0, x0 + IMG_W * region, n_in)
    y1 = rng.uniform(y0, y0 + IMG_H * region, n_in)
    w = H[2, 0] * x1 + H[2, 1] * y1 + H[2, 2]
    x2 = (H[0, 0] * x1 + H[0, 1] * y1 + H[0, 2]) / w + rng.normal(0, noise, n_in)
    y2 = (H[1, 0] * x1 + H[1, 1] * y1 + H[1, 2]) / w + rng.normal(0, noise, n_in)
    inl = np.stack([x1, y1, x2, y2], axis=1)
    out = np.stack([rng.uniform(0, IMG_W, n_out), rng.uniform(0, IMG_H, n_out),
                    rng.uniform(0, IMG_W, n_out), rng.uniform(0, IMG_H, n_out)], axis=1)
    corr = np.concatenate([inl, out])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(n)
    return np.ascontiguousarray(corr[perm]), truth[perm], H.copy(), 2.0


def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = (math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll),
                              math.sin(roll))
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def two_view_geometry(focal: float = 1000.0, yaw: float = 0.12, pitch: float = 0.03, roll: float = 0.02,
                      t=(1.0, 0.1, 0.15)):
    """Calibration, relative pose and F_gt (x2^T F x1 = 0, unit Frobenius norm)."""
    K = np.array([[focal, 0, IMG_W / 2], [0, focal, IMG_H / 2], [0, 0, 1.0]])
    R = _rot(yaw, pitch, roll)
    t = np.asarray(t, dtype=float)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return K, R, t, F / np.linalg.norm(F)


def problem_f(n: int = 10_000, outlier_ratio: float = 0.8, seed: int = DEFAULT_SEED, noise: float = 0.5):
    """Fundamental-matrix problem (BASELINE configs[3]): a random 3-D scene seen
    by two calibrated cameras.  Returns correspondences (n, 4) = (x1, y1, x2,
    y2), inlier truth mask, F_gt and the inlier threshold (px, Sampson)."""
    rng = np.random.default_rng(seed)
    K, R, t, F = two_view_geometry()
    n_out = int(round(n * outlier_ratio))
    n_in = n - n_out
    pts = []
    while sum(len(p) for p in pts) < n_in:
        m = 2 * n_in
        X = np.stack([rng.uniform(-5, 5, m), rng.uniform(-4, 4, m), rng.uniform(6, 16, m)], axis=1)
        p1 = X @ K.T
        X2 = X @ R.T + t
        p2 = X2 @ K.T
        ok = (X2[:, 2] > 0.1)
        u1, v1 = p1[:, 0] / p1[:, 2], p1[:, 1] / p1[:, 2]
        u2, v2 = p2[:, 0] / p2[:, 2], p2[:, 1] / p2[:, 2]
        ok &= (u1 >= 0) & (u1 < IMG_W) & (v1 >= 0) & (v1 < IMG_H) & (u2 >= 0) & (u2 < IMG_W) & (v2 >= 0) & (v2 < IMG_H)
        pts.append(np.stack([u1, v1, u2, v2], axis=1)[ok])
    inl = np.concatenate(pts)[:n_in]
    inl = inl + rng.normal(0, noise, inl.shape)
    out = np.stack([rng.uniform(0, IMG_W, n_out), rng.uniform(0, IMG_H, n_out),
                    rng.uniform(0, IMG_W, n_out), rng.uniform(0, IMG_H, n_out)], axis=1)
    corr = np.concatenate([inl, out])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(n)
    return np.ascontiguousarray(corr[perm]), truth[perm], F, 1.0


def problem_e(n: int = 10_000, outlier_ratio: float = 0.8, seed: int = DEFAULT_SEED, noise: float = 0.5):
    """Essential-matrix problem: problem_f's scene and pixel correspondences
    with the calibration of two_view_geometry (both cameras).  Returns
    correspondences (n, 4) in pixels, inlier truth mask, K, E_gt (normalised
    coordinates: x^2^T E x^1 = 0 with x^ = K^-1 x, unit Frobenius norm) and the
    inlier threshold (px)."""
    corr, truth, _, thr = problem_f(n, outlier_ratio, seed, noise)
    K, R, t, _ = two_view_geometry()
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return corr, truth, K, E / np.linalg.norm(E), thr


def gravity_geometry(seed: int = DEFAULT_SEED, focal: float = 1000.0):
    """Calibration, gravity-alignment rotations and relative pose of a
    two-view problem with known gravity: G1, G2 are seeded random rotations
    (yaw, pitch, roll within +-0.15 rad: cameras held roughly upright), the
    relative pose in the aligned frames is a rotation about y (+-0.3 rad) and
    a unit translation.  Returns K, G1, G2, R, t (camera frames:
    R = G2^T R_y G1, t = G2^T t') and E_gt = [t]x R at unit Frobenius norm."""
    rng = np.random.default_rng([seed, 0x67726176])
    K = np.array([[focal, 0, IMG_W / 2], [0, focal, IMG_H / 2], [0, 0, 1.0]])
    G1 = _rot(*rng.uniform(-0.15, 0.15, 3))
    G2 = _rot(*rng.uniform(-0.15, 0.15, 3))
    th = rng.uniform(0.05, 0.3) * (1.0 if rng.uniform() < 0.5 else -1.0)
    Ry = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])
    ta = np.array([1.0, rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)])
    ta /= np.linalg.norm(ta)
    R = G2.T @ Ry @ G1
    t = G2.T @ ta
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return K, G1, G2, R, t, E / np.linalg.norm(E)


def problem_g(n: int = 10_000, outlier_ratio: float = 0.8, seed: int = DEFAULT_SEED, noise: float = 0.5):
    """Essential-matrix problem with known gravity: problem_e's scene (the
    same 3-D box, image size, calibration, noise and outliers; inlier
    threshold 1 px) seen by the cameras of gravity_geometry(seed).  Returns
    correspondences (n, 4) in pixels, inlier truth mask, K (both cameras),
    G1, G2 and E_gt (normalised coordinates, unit Frobenius norm)."""
    rng = np.random.default_rng(seed)
    K, G1, G2, R, t, E = gravity_geometry(seed)
    n_out = int(round(n * outlier_ratio))
    n_in = n - n_out
    pts = []
    while sum(len(p) for p in pts) < n_in:
        m = 2 * n_in + 8
        X = np.stack([rng.uniform(-5, 5, m), rng.uniform(-4, 4, m), rng.uniform(6, 16, m)], axis=1)
        p1 = X @ K.T
        X2 = X @ R.T + t
        p2 = X2 @ K.T
        ok = (X2[:, 2] > 0.1)
        u1, v1 = p1[:, 0] / p1[:, 2], p1[:, 1] / p1[:, 2]
        u2, v2 = p2[:, 0] / p2[:, 2], p2[:, 1] / p2[:, 2]
        ok &= (u1 >= 0) & (u1 < IMG_W) & (v1 >= 0) & (v1 < IMG_H) & (u2 >= 0) & (u2 < IMG_W) & (v2 >= 0) & (v2 < IMG_H)
        pts.append(np.stack([u1, v1, u2, v2], axis=1)[ok])
    inl = np.concatenate(pts)[:n_in]
    inl = inl + rng.normal(0, noise, inl.shape)
    out = np.stack([rng.uniform(0, IMG_W, n_out), rng.uniform(0, IMG_H, n_out),
                    rng.uniform(0, IMG_W, n_out), rng.uniform(0, IMG_H, n_out)], axis=1)
    corr = np.concatenate([inl, out])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(n)
    return np.ascontiguousarray(corr[perm]), truth[perm], K, G1, G2, E


def affine_of_h(H: np.ndarray, x1, y1):
    """The local affine map of the homography H at the points (x1, y1): the
    Jacobian of x -> H x, (n, 2, 2)."""
    x1 = np.asarray(x1, dtype=float)
    y1 = np.asarray(y1, dtype=float)
    s = H[2, 0] * x1 + H[2, 1] * y1 + H[2, 2]
    x2 = (H[0, 0] * x1 + H[0, 1] * y1 + H[0, 2]) / s
    y2 = (H[1, 0] * x1 + H[1, 1] * y1 + H[1, 2]) / s
    A = np.empty(x1.shape + (2, 2))
    A[..., 0, 0] = (H[0, 0] - x2 * H[2, 0]) / s
    A[..., 0, 1] = (H[0, 1] - x2 * H[2, 1]) / s
    A[..., 1, 0] = (H[1, 0] - y2 * H[2, 0]) / s
    A[..., 1, 1] = (H[1, 1] - y2 * H[2, 1]) / s
    return A


def problem_hs(n: int = 5_000, outlier_ratio: float = 0.5, seed: int = DEFAULT_SEED, noise: float = 0.5,
               scale_noise: float = 0.05, angle_noise: float = math.radians(2.0), H: np.ndarray = H_GT):
    """Homography problem with SIFT columns: problem_h's rows (the same rows
    bit for bit) plus q1, q2, alpha1, alpha2.  Inliers: q1 log-uniform in
    [2, 30], alpha1 uniform in [-pi, pi), alpha2 and q2 from the true local
    affine map A of H at (x1, y1) -- the direction of A d1 and q1 sqrt(det A)
    -- with Gaussian noise `angle_noise` (radians) on alpha2 and lognormal
    noise `scale_noise` on q2.  Outliers: all four columns random.  Returns
    correspondences (n, 8), inlier truth mask, ground-truth H and the inlier
    threshold (px)."""
    corr, truth, Hgt, thr = problem_h(n, outlier_ratio, seed, noise, H)
    rng = np.random.default_rng([seed, 0x73696674])
    q1 = np.exp(rng.uniform(math.log(2.0), math.log(30.0), n))
    a1 = rng.uniform(-math.pi, math.pi, n)
    q2 = np.exp(rng.uniform(math.log(2.0), math.log(30.0), n))
    a2 = rng.uniform(-math.pi, math.pi, n)
    en = rng.normal(0.0, 1.0, n)
    sn = rng.normal(0.0, 1.0, n)
    A = affine_of_h(H, corr[:, 0], corr[:, 1])
    dx, dy = np.cos(a1), np.sin(a1)
    tx = A[:, 0, 0] * dx + A[:, 0, 1] * dy
    ty = A[:, 1, 0] * dx + A[:, 1, 1] * dy
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    a2_in = np.arctan2(ty, tx) + angle_noise * en
    q2_in = q1 * np.sqrt(np.abs(det)) * np.exp(scale_noise * sn)
    a2 = np.where(truth, a2_in, a2)
    q2 = np.where(truth, q2_in, q2)
    return np.ascontiguousarray(np.column_stack([corr, q1, q2, a1, a2])), truth, Hgt, thr


def problem_match(n: int = 1_000, shared: int = 400, seed: int = DEFAULT_SEED, desc_noise: float = 40.0,
                  dim: int = 128):
    """Two images' keypoints and uint8 descriptors, for match_descriptors and
    the estimators behind it.  Each image has n keypoints (x, y, size,
    angle_deg); `shared` of them are the same scene points: related by
    problem_hs's geometry (H_GT, its pixel, size and orientation noise), their
    descriptors one uniform random byte vector per scene point plus Gaussian
    noise of `desc_noise` per image, rounded and clipped to 0..255.  The other
    n - shared keypoints of each image are independent (uniform positions
    and descriptors).  Image 2 is permuted.

    Returns (kp1 (n, 4), desc1 (n, dim) uint8, kp2, desc2, pairs (shared, 2)
    int64 rows (i, j) sorted by i, H_gt)."""
    if not 0 <= shared <= n:
        raise ValueError("need 0 <= shared <= n")
    c8, _, Hgt, _ = problem_hs(shared, 0.0, seed) if shared else (np.zeros((0, 8)), None, H_GT.copy(), None)
    rng = np.random.default_rng([seed, 0x6d617463])
    rest = n - shared

    def independent(k):
        return np.column_stack([rng.uniform(0, IMG_W, k), rng.uniform(0, IMG_H, k),
                                np.exp(rng.uniform(math.log(2.0), math.log(30.0), k)),
                                np.degrees(rng.uniform(-math.pi, math.pi, k))])

    kp1 = np.concatenate([np.column_stack([c8[:, 0], c8[:, 1], c8[:, 4], np.degrees(c8[:, 6])]), independent(rest)])
    kp2 = np.concatenate([np.column_stack([c8[:, 2], c8[:, 3], c8[:, 5], np.degrees(c8[:, 7])]), independent(rest)])
    base = rng.integers(0, 256, (shared, dim)).astype(np.float64)

    def noisy():
        return np.clip(np.rint(base + rng.normal(0.0, desc_noise, base.shape)), 0, 255).astype(np.uint8)

    desc1 = np.concatenate([noisy(), rng.integers(0, 256, (rest, dim), dtype=np.uint8)])
    desc2 = np.concatenate([noisy(), rng.integers(0, 256, (rest, dim), dtype=np.uint8)])
    # image 1 is shuffled too, so that the shared keypoints are not its first rows
    p1, p2 = rng.permutation(n), rng.permutation(n)
    inv1, inv2 = np.empty(n, np.int64), np.empty(n, np.int64)
    inv1[p1] = np.arange(n)
    inv2[p2] = np.arange(n)
    pairs = np.stack([inv1[:shared], inv2[:shared]], axis=1)
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
    return (np.ascontiguousarray(kp1[p1]), np.ascontiguousarray(desc1[p1]), np.ascontiguousarray(kp2[p2]),
            np.ascontiguousarray(desc2[p2]), pairs, Hgt)


def problem_match_repeated(n: int = 1_000, groups: int = 100, repeats: int = 3, seed: int = DEFAULT_SEED,
                           desc_noise: float = 20.0, dim: int = 256):
    """problem_match with REPEATED structure (facades, tiles, windows), for
    knn_descriptors and matches_from_knn.  groups * repeats of each image's n
    keypoints are shared scene points; the `repeats` scene points of a group
    share ONE base descriptor (one uniform random byte vector per group) but
    lie at independent positions: problem_hs's geometry under H_GT, as
    problem_match's shared keypoints.  Each image adds its own Gaussian
    descriptor noise of `desc_noise`, rounded and clipped to 0..255.  The other
    keypoints of each image are independent; both images are permuted.  A
    shared keypoint's nearest `repeats` neighbours are therefore the copies of
    its group, at about equal distances, and the true one is any of them.
    The distances inside a group scatter by about sqrt(2 / dim) of their mean
    whatever the noise: at the default dim of 256 the smallest ratio of two of
    them stays near 0.75, clear of the 0.8^2 = 0.64 of the usual ratio test
    (at dim 128 it comes down to 0.62 in one row of 300), while the ratio to
    the first neighbour outside the group is near 0.12.

    Returns problem_match's tuple: (kp1 (n, 4), desc1 (n, dim) uint8, kp2,
    desc2, pairs (groups * repeats, 2) int64 rows (i, j) of the same scene
    point sorted by i, H_gt)."""
    shared = groups * repeats
    if groups < 0 or repeats < 1 or shared > n:
        raise ValueError("need groups >= 0, repeats >= 1 and groups * repeats <= n")
    c8, _, Hgt, _ = problem_hs(shared, 0.0, seed) if shared else (np.zeros((0, 8)), None, H_GT.copy(), None)
    rng = np.random.default_rng([seed, 0x72657065])
    rest = n - shared

    def independent(k):
        return np.column_stack([rng.uniform(0, IMG_W, k), rng.uniform(0, IMG_H, k),
                                np.exp(rng.uniform(math.log(2.0), math.log(30.0), k)),
                                np.degrees(rng.uniform(-math.pi, math.pi, k))])

    kp1 = np.concatenate([np.column_stack([c8[:, 0], c8[:, 1], c8[:, 4], np.degrees(c8[:, 6])]), independent(rest)])
    kp2 = np.concatenate([np.column_stack([c8[:, 2], c8[:, 3], c8[:, 5], np.degrees(c8[:, 7])]), independent(rest)])
    # scene point s belongs to group s // repeats
    base = np.repeat(rng.integers(0, 256, (groups, dim)).astype(np.float64), repeats, axis=0)

    def noisy():
        return np.clip(np.rint(base + rng.normal(0.0, desc_noise, base.shape)), 0, 255).astype(np.uint8)

    desc1 = np.concatenate([noisy(), rng.integers(0, 256, (rest, dim), dtype=np.uint8)])
    desc2 = np.concatenate([noisy(), rng.integers(0, 256, (rest, dim), dtype=np.uint8)])
    p1, p2 = rng.permutation(n), rng.permutation(n)
    inv1, inv2 = np.empty(n, np.int64), np.empty(n, np.int64)
    inv1[p1] = np.arange(n)
    inv2[p2] = np.arange(n)
    pairs = np.stack([inv1[:shared], inv2[:shared]], axis=1)
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
    return (np.ascontiguousarray(kp1[p1]), np.ascontiguousarray(desc1[p1]), np.ascontiguousarray(kp2[p2]),
            np.ascontiguousarray(desc2[p2]), pairs, Hgt)
