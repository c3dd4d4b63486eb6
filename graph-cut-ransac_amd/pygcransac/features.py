"""Feature front-end and output warp of the example notebook flow
(examples/utils.py:5-49 and :92-123 of the reference).

The reference takes cv2.KeyPoint lists.  cv2 is optional here: any object
with .pt, .size and .angle works, and so does an (N, 4) array of
(x, y, size, angle_degrees) rows (angle -1 = none, OpenCV's convention).
`perspective_warp` rectifies an image with the estimated homography on the
GPU (a HIP resampling kernel behind gcr_warp_perspective), cv2-free.

`match_descriptors` is the step before the estimators: exact 2-nearest-
neighbour matching of uint8 (SIFT-style) descriptors on the GPU's int8 matrix
cores (gcr_match_descriptors, csrc/match.h), with the ratio test and the
mutual check.  `quantize_descriptors` brings float descriptors to uint8 and
`correspondences_from_matches` builds the estimators' rows from the matches.
`match_descriptors_guided` is the matcher's second run, after the estimator:
the same search among the pairs that agree with the estimated homography or
fundamental matrix (gcr_match_descriptors_guided, csrc/match_geo.h);
`fundamental_from_essential` brings an essential matrix to that form.
`DescriptorSet` keeps one image's descriptors (and keypoints) on the device:
`a.match(b)`, `a.match_guided(b, ...)` and `match_pairs` give the array
functions' results without their uploads, with the ratio test, the mutual check
and the row selection on the GPU too (csrc/match_sets.h, csrc/match_select.h).
`knn_descriptors` (and `DescriptorSet.knn`) return every row's k nearest
neighbours (gcr_knn_descriptors, csrc/match_knn.h) and `matches_from_knn` turns
them into one-to-many matches: on repeated structure, where the second
neighbour is another copy of the true one, the ratio test moves to the end of
the group of equally good candidates.
"""
from __future__ import annotations

import numpy as np

__all__ = ["scale_features_from_sift", "orientation_features_from_sift", "keypoints_to_array", "perspective_warp",
           "warp_geometry", "BORDER_CONSTANT", "BORDER_REPLICATE", "match_descriptors", "quantize_descriptors",
           "correspondences_from_matches", "match_descriptors_guided", "fundamental_from_essential", "DescriptorSet",
           "match_pairs", "knn_descriptors", "matches_from_knn", "verify_pairs"]

# OpenCV's border codes (cv2.BORDER_CONSTANT = 0, cv2.BORDER_REPLICATE = 1)
BORDER_CONSTANT, BORDER_REPLICATE = 0, 1


def keypoints_to_array(keypoints) -> np.ndarray:
    """(N, 4) float64 rows (x, y, size, angle_deg) from cv2-style keypoints or an array."""
    if isinstance(keypoints, np.ndarray):
        a = np.asarray(keypoints, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] < 4:
            raise ValueError("keypoint array must have shape (N, 4): x, y, size, angle (degrees)")
        return a[:, :4]
    rows = [(float(kp.pt[0]), float(kp.pt[1]), float(kp.size), float(kp.angle)) for kp in keypoints]
    return np.array(rows, dtype=np.float64).reshape(-1, 4)


def scale_features_from_sift(keypoints) -> np.ndarray:
    """One (x, y, size) row per distinct integer pixel, first keypoint wins,
    in first-seen order (utils.py:5-26: dict keyed by (int(x), int(y)))."""
    kp = keypoints_to_array(keypoints)
    unique = {}
    for row in kp:
        key = (int(row[0]), int(row[1]))          # int() truncates toward zero, as in Python
        if key not in unique:
            unique[key] = row
    if not unique:
        return np.array([])
    return np.array([[r[0], r[1], r[2]] for r in unique.values()])


def orientation_features_from_sift(keypoints):
    """(x, y, angle in radians) for every keypoint with an angle (!= -1) and the
    matching sizes 0.5 * size (utils.py:29-49)."""
    kp = keypoints_to_array(keypoints)
    feats, sizes = [], []
    for row in kp:
        if row[3] != -1:
            feats.append([row[0], row[1], np.deg2rad(row[3])])
            sizes.append(0.5 * row[2])
    return np.array(feats), np.array(sizes)


def warp_geometry(h: int, w: int, H):
    """Output frame of perspective_warp (utils.py:107-118): the image corners
    (0,0), (w,0), (w,h), (0,h) through H, their bounding box, the output size
    (ceil of its extent) and the translated homography T @ H that moves the
    box's minimum corner to the origin.

    Returns (H_translated (3, 3), (out_w, out_h), (min_x, min_y))."""
    H = np.asarray(H, dtype=np.float64).reshape(3, 3)
    corners = np.array([[0, 0, 1], [w, 0, 1], [w, h, 1], [0, h, 1]]).T
    wc = H @ corners
    wc = wc[:2] / wc[2]
    min_x, min_y = wc.min(axis=1)
    max_x, max_y = wc.max(axis=1)
    size = (int(np.ceil(max_x - min_x)), int(np.ceil(max_y - min_y)))
    translation = np.array([[1, 0, -min_x], [0, 1, -min_y], [0, 0, 1]])
    return translation @ H, size, (min_x, min_y)


def perspective_warp(img, H, border_mode=BORDER_CONSTANT, border_value=(255, 255, 255), device=None):
    """Warp `img` with homography H into an automatically sized frame
    (utils.py:92-123).  img: (h, w) or (h, w, c) uint8 / float32 array, c <= 4.

    Returns (warped_img, H_translated, (min_x, min_y)) like the reference.
    Resampling as cv2.warpPerspective's INTER_LINEAR: every output pixel takes
    the bilinear sample at inv(H_translated) (x, y, 1); neighbours outside the
    image take `border_value` (BORDER_CONSTANT) or the nearest edge pixel
    (BORDER_REPLICATE).  cv2 blends in fixed point (5-bit sub-pixel
    positions), this kernel in float32: uint8 outputs can differ from cv2's by
    one grey level at sub-pixel positions."""
    import ctypes as C

    from . import _native as N

    a = np.asarray(img)
    if a.ndim not in (2, 3) or (a.ndim == 3 and not 1 <= a.shape[2] <= 4):
        raise ValueError("img must have shape (h, w) or (h, w, c) with 1 <= c <= 4")
    if a.dtype == np.uint8:
        dtype = 0
    elif a.dtype in (np.float32, np.float64):
        a, dtype = a.astype(np.float32), 1
    else:
        raise ValueError(f"unsupported image dtype {a.dtype} (uint8 or float32)")
    if border_mode not in (BORDER_CONSTANT, BORDER_REPLICATE):
        raise ValueError("border_mode must be BORDER_CONSTANT (0) or BORDER_REPLICATE (1)")
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    Ht, (ow, oh), mins = warp_geometry(h, w, H)
    M = np.ascontiguousarray(np.linalg.inv(Ht), dtype=np.float64)
    bv = np.zeros(4)
    vals = np.atleast_1d(np.asarray(border_value, dtype=np.float64))
    bv[:min(4, vals.size)] = vals[:4]
    if vals.size == 1:
        bv[:] = vals[0]
    src = np.ascontiguousarray(a)
    out = np.empty((oh, ow) if a.ndim == 2 else (oh, ow, ch), dtype=src.dtype)
    dp = C.POINTER(C.c_double)
    N.check(N.lib.gcr_warp_perspective(N.context(device), src.ctypes.data, h, w, ch, dtype, M.ctypes.data_as(dp),
                                       int(border_mode), bv.ctypes.data_as(dp), out.ctypes.data, oh, ow))
    return out, Ht, mins


def quantize_descriptors(desc, scale: float = 512.0) -> np.ndarray:
    """uint8 descriptors from float ones: ``clip(rint(scale * x), 0, 255)``.
    The default scale is the usual one for unit-norm 128-d descriptors (SIFT,
    RootSIFT), whose components rarely pass 0.5."""
    a = np.asarray(desc, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("descriptors must have shape (N, dim)")
    if not np.isfinite(a).all():
        raise ValueError("descriptors must be finite")
    return np.clip(np.rint(float(scale) * a), 0.0, 255.0).astype(np.uint8)


def _as_descriptors(desc, name):
    a = np.asarray(desc)
    if a.dtype != np.uint8:
        raise ValueError(f"{name} must be a uint8 array, got {a.dtype}; quantize_descriptors() converts float "
                         "descriptors")
    if a.ndim != 2:
        raise ValueError(f"{name} must have shape (N, dim), got {a.shape}")
    return np.ascontiguousarray(a)


def _nearest_two(d1, d2, backend, device):
    """idx, dist, idx2, dist2 (uint32, one per row of d1) by the engine."""
    from . import _native as N

    n1, dim = d1.shape
    out = [np.empty(n1, dtype=np.uint32) for _ in range(4)]
    ptrs = [o.ctypes.data for o in out]
    if backend == "host":
        import os

        threads = max(1, min(16, os.cpu_count() or 1))
        N.check(N.lib.gcr_host_match_descriptors(d1.ctypes.data, n1, d2.ctypes.data, d2.shape[0], dim, threads, *ptrs))
    else:
        N.check(N.lib.gcr_match_descriptors(N.context(device), d1.ctypes.data, n1, d2.ctypes.data, d2.shape[0], dim,
                                            *ptrs, None))
    return out


def match_descriptors(desc1, desc2, ratio=0.8, mutual=True, *, backend="gpu", device=None):
    """Match two sets of uint8 descriptors: exact nearest and second-nearest
    neighbour of every row of ``desc1`` among the rows of ``desc2`` under the
    squared Euclidean distance (an integer; on equal distances the lower index
    is nearer), Lowe's ratio test and the mutual-nearest check.

    ``desc1`` is (n1, dim) and ``desc2`` (n2, dim), both uint8 (anything else
    is a ValueError: ``quantize_descriptors`` converts float descriptors);
    ``dim`` is a multiple of 32 in 32..512.  A pair (i, j) passes the ratio
    test iff ``float(dist) < (ratio * ratio) * float(dist2)`` in float64, where
    dist2 is the distance to i's second neighbour; with no second neighbour
    (n2 == 1) it fails.  ``ratio=None`` skips the test.  ``mutual=True`` keeps
    (i, j) iff j is i's nearest and i is j's nearest (a second matching with
    the arguments swapped, the same tie rule).  ``backend="gpu"`` runs the HIP
    kernels (csrc/match.hip: int8 matrix cores, exact), ``backend="host"`` the
    plain-loop definition on up to 16 threads, without a GPU; both give the
    same bytes.  Binary descriptors (ORB, BRIEF) packed into bytes match in the
    exact Hamming order as ``match_descriptors(np.unpackbits(a, axis=1),
    np.unpackbits(b, axis=1))``: on 0 / 1 components the squared Euclidean
    distance is the Hamming distance.

    Returns ``(matches, ratios)``: ``matches`` (M, 2) int64 rows (i, j) sorted
    by i, ``ratios`` (M,) float64 with sqrt(dist / dist2) (1.0 for 0 / 0 and
    where there is no second neighbour).  ``-ratios`` is a valid
    ``probabilities`` for the estimators' ``sampler=1`` (PROSAC): a quality
    score per correspondence, higher is better."""
    d1 = _as_descriptors(desc1, "desc1")
    d2 = _as_descriptors(desc2, "desc2")
    if d1.shape[1] != d2.shape[1]:
        raise ValueError(f"desc1 and desc2 differ in dimension: {d1.shape[1]} and {d2.shape[1]}")
    if d1.shape[1] % 32 or not 32 <= d1.shape[1] <= 512:
        raise ValueError(f"the descriptor dimension must be a multiple of 32 in 32..512, got {d1.shape[1]}")
    if d1.shape[0] == 0 or d2.shape[0] == 0:
        raise ValueError("desc1 and desc2 need at least one row each")
    if backend not in ("gpu", "host"):
        raise ValueError(f"backend must be 'gpu' or 'host', got {backend!r}")
    if ratio is not None and not (np.isfinite(ratio) and ratio > 0):
        raise ValueError("ratio must be None or a finite number > 0")
    idx, dist, idx2, dist2 = _nearest_two(d1, d2, backend, device)
    none = idx2 == 0xFFFFFFFF
    fd, fd2 = dist.astype(np.float64), dist2.astype(np.float64)
    ratios = np.ones(len(idx), dtype=np.float64)
    ok = ~none & (fd2 > 0)
    ratios[ok] = np.sqrt(fd[ok] / fd2[ok])
    keep = np.ones(len(idx), dtype=bool)
    if ratio is not None:
        keep &= ~none & (fd < (float(ratio) * float(ratio)) * fd2)
    if mutual:
        back = _nearest_two(d2, d1, backend, device)[0]
        keep &= back[idx] == np.arange(len(idx), dtype=np.uint32)
    rows = np.nonzero(keep)[0]
    matches = np.stack([rows.astype(np.int64), idx[rows].astype(np.int64)], axis=1)
    return matches, ratios[rows]


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 8:
        raise ValueError(f"k must be an integer in 1..8, got {k!r}")
    return int(k)


def knn_descriptors(desc1, desc2, k, *, backend="gpu", device=None):
    """The exact ``k`` nearest neighbours of every row of ``desc1`` among the
    rows of ``desc2``: ``match_descriptors``'s descriptors, distance and order
    (squared Euclidean, an integer; on equal distances the lower index is
    nearer), ``k`` in 1..8.

    ``desc1`` is (n1, dim) and ``desc2`` (n2, dim), both uint8 (anything else
    is a ValueError: ``quantize_descriptors`` converts float descriptors);
    ``dim`` is a multiple of 32 in 32..512.  ``backend="gpu"`` runs the HIP
    kernels (csrc/match_knn.hip: int8 matrix cores, exact), ``backend="host"``
    the plain-loop definition on up to 16 threads, without a GPU; both give the
    same bytes.

    Returns ``(idx, dist)``, both (n1, k) uint32: row i holds the indices and
    the distances of i's neighbours, nearest first; 0xFFFFFFFF in both from
    position n2 on where ``desc2`` has fewer than ``k`` rows.  For ``k=2`` the
    columns are the nearest and second-nearest neighbour ``match_descriptors``
    works on.  ``matches_from_knn`` builds one-to-many matches from them."""
    from . import _native as N

    d1 = _as_descriptors(desc1, "desc1")
    d2 = _as_descriptors(desc2, "desc2")
    if d1.shape[1] != d2.shape[1]:
        raise ValueError(f"desc1 and desc2 differ in dimension: {d1.shape[1]} and {d2.shape[1]}")
    if d1.shape[1] % 32 or not 32 <= d1.shape[1] <= 512:
        raise ValueError(f"the descriptor dimension must be a multiple of 32 in 32..512, got {d1.shape[1]}")
    if d1.shape[0] == 0 or d2.shape[0] == 0:
        raise ValueError("desc1 and desc2 need at least one row each")
    if backend not in ("gpu", "host"):
        raise ValueError(f"backend must be 'gpu' or 'host', got {backend!r}")
    k = _check_k(k)
    n1, dim = d1.shape
    idx = np.empty((n1, k), dtype=np.uint32)
    dist = np.empty((n1, k), dtype=np.uint32)
    if backend == "host":
        import os

        threads = max(1, min(16, os.cpu_count() or 1))
        N.check(N.lib.gcr_host_knn_descriptors(d1.ctypes.data, n1, d2.ctypes.data, d2.shape[0], dim, k, threads,
                                               idx.ctypes.data, dist.ctypes.data))
    else:
        N.check(N.lib.gcr_knn_descriptors(N.context(device), d1.ctypes.data, n1, d2.ctypes.data, d2.shape[0], dim, k,
                                          idx.ctypes.data, dist.ctypes.data, None))
    return idx, dist


def matches_from_knn(idx, dist, ratio=0.8, max_group=None):
    """One-to-many matches from ``knn_descriptors``'s ``(idx, dist)``: the
    ratio test generalised to a GROUP of equally good candidates.  Where a
    descriptor repeats g times in the other image (facades, tiles, windows) the
    first g neighbours are at about the same distance and the gap follows
    them, so Lowe's test between the first and the second fails although the
    true match is among the g.

    For row i and a group size g = 1 .. min(k - 1, max_group) the gap holds
    iff neighbour g exists (is not 0xFFFFFFFF) and ``float(dist[i, g - 1]) <
    (ratio * ratio) * float(dist[i, g])`` in float64, ``match_descriptors``'s
    comparison.  The row's group is the SMALLEST such g, and the row gives the
    g matches (i, idx[i, 0]), ..., (i, idx[i, g - 1]); a row without a gap
    gives none.  ``max_group=None`` allows every g up to k - 1.

    Returns ``(matches, group, ratios)``: ``matches`` (M, 2) int64 rows (i, j)
    sorted by i, then by rank; ``group`` (M,) int64, the size g of the group a
    match belongs to; ``ratios`` (M,) float64, sqrt(dist[i, g - 1] / dist[i, g])
    of its row.  For k = 2 this is ``match_descriptors(ratio=ratio,
    mutual=False)``, rows and ratios.  ``1.0 / group`` is a valid
    ``probabilities`` for the estimators' ``sampler=3`` (guided sampling, with
    ``guided_stop=True``): one of g equally good candidates is the true one with
    probability 1 / g at most."""
    ix, ds = np.asarray(idx), np.asarray(dist)
    if ix.ndim != 2 or ix.shape != ds.shape:
        raise ValueError(f"idx and dist must have the same shape (n, k), got {ix.shape} and {ds.shape}")
    if ix.dtype != np.uint32 or ds.dtype != np.uint32:
        raise ValueError("idx and dist must be uint32 arrays (knn_descriptors' outputs)")
    n, k = ix.shape
    if not 1 <= k <= 8:
        raise ValueError(f"k (the number of columns) must be in 1..8, got {k}")
    if not (isinstance(ratio, (int, float, np.integer, np.floating)) and np.isfinite(ratio) and ratio > 0):
        raise ValueError("ratio must be a finite number > 0")
    if max_group is None:
        gmax = k - 1
    else:
        if isinstance(max_group, bool) or not isinstance(max_group, (int, np.integer)) or max_group < 1:
            raise ValueError(f"max_group must be None or an integer >= 1, got {max_group!r}")
        gmax = min(k - 1, int(max_group))
    rr = float(ratio) * float(ratio)
    fd = ds.astype(np.float64)
    grp = np.zeros(n, dtype=np.int64)                     # 0: no gap yet
    for g in range(1, gmax + 1):
        gap = (ix[:, g] != 0xFFFFFFFF) & (fd[:, g - 1] < rr * fd[:, g])
        grp[(grp == 0) & gap] = g
    rows = np.nonzero(grp)[0]
    g = grp[rows]
    i = np.repeat(rows, g)
    rank = np.arange(len(i), dtype=np.int64) - np.repeat(np.cumsum(g) - g, g)
    matches = np.stack([i.astype(np.int64), ix[i, rank].astype(np.int64)], axis=1).reshape(-1, 2)
    row_ratio = np.sqrt(fd[rows, g - 1] / fd[rows, np.minimum(g, k - 1)])
    return matches, np.repeat(g, g), np.repeat(row_ratio, g)


def _positions(kp, name):
    """(N, 2) contiguous float64 (x, y) from keypoints (keypoints_to_array's columns 0 and 1) or an (N, 2) array."""
    if isinstance(kp, np.ndarray) and kp.ndim == 2 and kp.shape[1] == 2:
        a = np.asarray(kp, dtype=np.float64)
    else:
        a = keypoints_to_array(kp)[:, :2]
    if not np.isfinite(a).all():
        raise ValueError(f"{name} has a non-finite position")
    return np.ascontiguousarray(a)


_GUIDED_KINDS = {"homography": 3, "fundamental": 4}     # GCR_SOLVER_HOMOGRAPHY4, GCR_SOLVER_FUNDAMENTAL7


def _nearest_two_guided(d1, p1, d2, p2, kind, model, sq_threshold, reverse, backend, device):
    """idx, dist, idx2, dist2 (uint32): one per row of d1, or of d2 with reverse=1."""
    from . import _native as N

    n = d2.shape[0] if reverse else d1.shape[0]
    out = [np.empty(n, dtype=np.uint32) for _ in range(4)]
    ptrs = [o.ctypes.data for o in out]
    args = (d1.ctypes.data, d1.shape[0], p1.ctypes.data, d2.ctypes.data, d2.shape[0], p2.ctypes.data, d1.shape[1],
            kind, model.ctypes.data, float(sq_threshold), int(reverse))
    if backend == "host":
        import os

        threads = max(1, min(16, os.cpu_count() or 1))
        N.check(N.lib.gcr_host_match_descriptors_guided(*args, threads, *ptrs))
    else:
        N.check(N.lib.gcr_match_descriptors_guided(N.context(device), *args, *ptrs, None))
    return out


def match_descriptors_guided(desc1, desc2, kp1, kp2, model, kind, threshold, ratio=None, mutual=True,
                             max_distance=None, *, backend="gpu", device=None):
    """Guided matching, the matcher's second run once a model is known: keypoint
    j of image 2 competes for keypoint i of image 1 only if the pair agrees
    with ``model``.  This recovers the correspondences that the ratio test and
    the mutual check of ``match_descriptors`` had to drop as ambiguous.

    ``desc1`` / ``desc2`` as for ``match_descriptors``.  ``kp1`` / ``kp2`` are
    read as by ``keypoints_to_array`` (columns 0 and 1: x, y); an (N, 2) array
    of positions is accepted too; one keypoint per descriptor row.  ``model``
    is 3 x 3 and ``kind`` says what it is: ``"homography"`` (image 1 to image
    2; the residual is the squared transfer error in image 2) or
    ``"fundamental"`` (x2^T F x1 = 0; the squared Sampson distance) -- the
    residuals of findHomography and findFundamentalMatrix.  An essential
    matrix goes through ``fundamental_from_essential`` first.  The pair (i, j)
    is admissible iff its residual is <= ``threshold * threshold`` in float64;
    ``threshold`` is in pixels, finite and > 0.  The estimators' own inlier
    mask uses the wider bound ``(2.25 * t) * t`` for their ``threshold`` t (1.5 t
    in pixels), so ``threshold = 1.5 * t`` admits the pairs that the estimator
    would call inliers of ``model`` (up to the rounding of the two bounds).

    Among the admissible candidates the search is ``match_descriptors``'s:
    exact squared descriptor distances, the lower index on a tie.
    ``mutual=True`` (a second search from image 2's side over the same
    admissible pairs) keeps (i, j) iff each is the other's first admissible
    neighbour.  ``ratio`` defaults to None: the geometry does the
    disambiguation.  When given, ``match_descriptors``'s float64 rule applies
    to the best and the second-best ADMISSIBLE candidate; a row with a single
    admissible candidate passes, because nothing competes with it.
    ``max_distance`` (optional) keeps a pair only if its squared descriptor
    distance is <= max_distance; under a homography, where a false keypoint
    often has one random admissible candidate, it is the only protection.
    A row without an admissible candidate gives no match.

    Returns ``(matches, ratios)`` as ``match_descriptors``: (M, 2) int64 rows
    (i, j) sorted by i and (M,) float64 sqrt(dist / dist2), 1.0 for 0 / 0 and
    where there is no second admissible neighbour."""
    d1 = _as_descriptors(desc1, "desc1")
    d2 = _as_descriptors(desc2, "desc2")
    if d1.shape[1] != d2.shape[1]:
        raise ValueError(f"desc1 and desc2 differ in dimension: {d1.shape[1]} and {d2.shape[1]}")
    if d1.shape[1] % 32 or not 32 <= d1.shape[1] <= 512:
        raise ValueError(f"the descriptor dimension must be a multiple of 32 in 32..512, got {d1.shape[1]}")
    if d1.shape[0] == 0 or d2.shape[0] == 0:
        raise ValueError("desc1 and desc2 need at least one row each")
    if backend not in ("gpu", "host"):
        raise ValueError(f"backend must be 'gpu' or 'host', got {backend!r}")
    if kind not in _GUIDED_KINDS:
        raise ValueError(f"kind must be 'homography' or 'fundamental', got {kind!r}")
    p1, p2 = _positions(kp1, "kp1"), _positions(kp2, "kp2")
    if len(p1) != len(d1) or len(p2) != len(d2):
        raise ValueError(f"one keypoint per descriptor: kp1 has {len(p1)} rows for {len(d1)} descriptors, "
                         f"kp2 {len(p2)} for {len(d2)}")
    m = np.asarray(model, dtype=np.float64)
    if m.shape != (3, 3) or not np.isfinite(m).all():
        raise ValueError("model must be a finite 3 x 3 matrix")
    m = np.ascontiguousarray(m)
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError("threshold must be a finite number of pixels > 0")
    if ratio is not None and not (np.isfinite(ratio) and ratio > 0):
        raise ValueError("ratio must be None or a finite number > 0")
    if max_distance is not None and not max_distance >= 0:
        raise ValueError("max_distance must be None or a number >= 0")
    T = float(threshold) * float(threshold)
    code = _GUIDED_KINDS[kind]
    idx, dist, idx2, dist2 = _nearest_two_guided(d1, p1, d2, p2, code, m, T, 0, backend, device)
    found = idx != 0xFFFFFFFF
    none = idx2 == 0xFFFFFFFF
    fd, fd2 = dist.astype(np.float64), dist2.astype(np.float64)
    ratios = np.ones(len(idx), dtype=np.float64)
    ok = found & ~none & (fd2 > 0)
    ratios[ok] = np.sqrt(fd[ok] / fd2[ok])
    keep = found.copy()
    if ratio is not None:
        keep &= none | (fd < (float(ratio) * float(ratio)) * fd2)
    if max_distance is not None:
        keep &= fd <= float(max_distance)
    if mutual:
        back = _nearest_two_guided(d1, p1, d2, p2, code, m, T, 1, backend, device)[0]
        rows = np.nonzero(keep)[0]
        keep[rows] = back[idx[rows]] == rows.astype(np.uint32)
    rows = np.nonzero(keep)[0]
    matches = np.stack([rows.astype(np.int64), idx[rows].astype(np.int64)], axis=1)
    return matches, ratios[rows]


def _match_options(ratio, mutual, max_distance=None):
    from . import _native as N

    opt = N.MatchOptions()
    opt.has_ratio = int(ratio is not None)
    opt.rr = float(ratio) * float(ratio) if ratio is not None else 0.0
    opt.mutual = int(bool(mutual))
    opt.has_max_distance = int(max_distance is not None)
    opt.max_distance = float(max_distance) if max_distance is not None else 0.0
    return opt


class DescriptorSet:
    """One image's uint8 descriptors, resident on the GPU: uploaded once, with
    their norms and, when ``keypoints`` are given, the keypoint positions.

    ``desc`` is (n, dim) uint8 under ``match_descriptors``'s rules (n >= 1, dim
    a multiple of 32 in 32..512).  ``keypoints`` are read as
    ``match_descriptors_guided`` reads ``kp1``: one per descriptor row; they
    are needed by ``match_guided`` only.  ``device`` as everywhere.

    ``a.match(b)``, ``a.match_guided(b, ...)`` and ``match_pairs`` return what
    ``match_descriptors`` / ``match_descriptors_guided`` return for the same
    arrays, byte for byte, but the searches, the ratio test, the mutual check,
    the ratios and the row selection all run on the device, and one download
    of the matches ends the call: no descriptor crosses the bus again.  A set
    can stand on either side of a match, against itself too, any number of
    times.  ``a.knn(b, k)`` is ``knn_descriptors`` on the two resident sets.

    ``len(s)`` is the row count; ``s.dim``, ``s.has_keypoints``.  ``close()``
    frees the device memory (also at the end of a ``with`` block and on
    garbage collection); a closed set raises ValueError when used."""

    def __init__(self, desc, keypoints=None, *, device=None):
        from . import _native as N

        self._handle = None
        d = _as_descriptors(desc, "desc")
        if d.shape[1] % 32 or not 32 <= d.shape[1] <= 512:
            raise ValueError(f"the descriptor dimension must be a multiple of 32 in 32..512, got {d.shape[1]}")
        if d.shape[0] == 0:
            raise ValueError("desc needs at least one row")
        p = None
        if keypoints is not None:
            p = _positions(keypoints, "keypoints")
            if len(p) != len(d):
                raise ValueError(f"one keypoint per descriptor: keypoints has {len(p)} rows for {len(d)} descriptors")
        import ctypes as C

        self._n, self._dim, self._has_kp = int(d.shape[0]), int(d.shape[1]), p is not None
        self._positions = p                               # the host copy (verify_pairs builds its rows from it)
        self._ctx = N.context(device)                     # the context outlives the set: kept for the process
        out = C.c_void_p()
        N.check(N.lib.gcr_descriptors_create(self._ctx, d.ctypes.data, self._n, self._dim,
                                             None if p is None else p.ctypes.data, C.byref(out)))
        self._handle = out.value

    def __len__(self):
        return self._n

    @property
    def dim(self) -> int:
        return self._dim

    @property
    def has_keypoints(self) -> bool:
        return self._has_kp

    @property
    def closed(self) -> bool:
        return self._handle is None

    def close(self) -> None:
        h, self._handle = self._handle, None
        if h is not None:
            from . import _native as N

            N.lib.gcr_descriptors_destroy(h)

    def __enter__(self):
        self._open()
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        if self._handle is None:
            raise ValueError("the DescriptorSet is closed")
        return self._handle

    def _pair(self, other):
        """the two handles, after the checks every match of two sets makes"""
        if not isinstance(other, DescriptorSet):
            raise ValueError(f"a DescriptorSet matches another DescriptorSet, got {type(other).__name__}")
        ha, hb = self._open(), other._open()
        if self._dim != other._dim:
            raise ValueError(f"desc1 and desc2 differ in dimension: {self._dim} and {other._dim}")
        if self._ctx != other._ctx:
            raise ValueError("the two DescriptorSets live on different devices")
        return ha, hb

    def _run(self, call):
        """call(matches_ptr, ratios_ptr, cap, m_ptr) -> the (matches, ratios) tuple"""
        import ctypes as C

        from . import _native as N

        matches = np.empty((self._n, 2), dtype=np.uint32)
        ratios = np.empty(self._n, dtype=np.float64)
        m = C.c_size_t()
        N.check(call(matches.ctypes.data, ratios.ctypes.data, self._n, C.byref(m)))
        return matches[:m.value].astype(np.int64), ratios[:m.value].copy()

    def match(self, other, ratio=0.8, mutual=True):
        """``match_descriptors(desc_self, desc_other, ratio, mutual)`` on the two
        resident sets: the same rules, the same ``(matches, ratios)``."""
        from . import _native as N

        ha, hb = self._pair(other)
        if ratio is not None and not (np.isfinite(ratio) and ratio > 0):
            raise ValueError("ratio must be None or a finite number > 0")
        opt = _match_options(ratio, mutual)
        return self._run(lambda mp, rp, cap, m: N.lib.gcr_match_sets(self._ctx, ha, hb, opt, mp, rp, cap, m, None))

    def match_guided(self, other, model, kind, threshold, ratio=None, mutual=True, max_distance=None):
        """``match_descriptors_guided(desc_self, desc_other, kp_self, kp_other,
        model, kind, threshold, ratio, mutual, max_distance)`` on the two
        resident sets; both need keypoints."""
        from . import _native as N

        ha, hb = self._pair(other)
        if kind not in _GUIDED_KINDS:
            raise ValueError(f"kind must be 'homography' or 'fundamental', got {kind!r}")
        if not (self._has_kp and other._has_kp):
            raise ValueError("match_guided needs keypoints on both DescriptorSets")
        m = np.asarray(model, dtype=np.float64)
        if m.shape != (3, 3) or not np.isfinite(m).all():
            raise ValueError("model must be a finite 3 x 3 matrix")
        m = np.ascontiguousarray(m)
        if not (np.isfinite(threshold) and threshold > 0):
            raise ValueError("threshold must be a finite number of pixels > 0")
        if ratio is not None and not (np.isfinite(ratio) and ratio > 0):
            raise ValueError("ratio must be None or a finite number > 0")
        if max_distance is not None and not max_distance >= 0:
            raise ValueError("max_distance must be None or a number >= 0")
        T = float(threshold) * float(threshold)
        opt = _match_options(ratio, mutual, max_distance)
        code = _GUIDED_KINDS[kind]
        return self._run(lambda mp, rp, cap, mo: N.lib.gcr_match_sets_guided(self._ctx, ha, hb, code, m.ctypes.data, T,
                                                                             opt, mp, rp, cap, mo, None))


    def knn(self, other, k):
        """``knn_descriptors(desc_self, desc_other, k)`` on the two resident
        sets: the same ``(idx, dist)``, without the uploads."""
        from . import _native as N

        ha, hb = self._pair(other)
        k = _check_k(k)
        idx = np.empty((self._n, k), dtype=np.uint32)
        dist = np.empty((self._n, k), dtype=np.uint32)
        N.check(N.lib.gcr_knn_sets(self._ctx, ha, hb, k, idx.ctypes.data, dist.ctypes.data, None))
        return idx, dist


def match_pairs(sets, pairs, ratio=0.8, mutual=True):
    """``a.match(b, ratio, mutual)`` for many pairs of resident sets in one
    call: every pair is queued on the device, then one synchronisation and one
    download.  ``sets`` is a sequence of ``DescriptorSet`` on one device,
    ``pairs`` a sequence of index pairs (ia, ib) into it, the row side first; a
    set may appear in any number of pairs, on either side, and with itself.

    Returns a list of ``(matches, ratios)`` tuples, one per pair in the order
    of ``pairs``, each equal to ``sets[ia].match(sets[ib], ratio, mutual)``.
    An empty ``pairs`` gives ``[]``."""
    import ctypes as C

    from . import _native as N

    sets = list(sets)
    for s in sets:
        if not isinstance(s, DescriptorSet):
            raise ValueError(f"sets must hold DescriptorSets, got {type(s).__name__}")
    pr = np.asarray(pairs)
    if pr.size == 0:
        pr = np.zeros((0, 2), dtype=np.int64)
    if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer):
        raise ValueError("pairs must be a sequence of integer pairs (ia, ib)")
    if pr.size and (pr.min() < 0 or pr.max() >= len(sets)):
        raise ValueError(f"pairs index past the {len(sets)} sets")
    if ratio is not None and not (np.isfinite(ratio) and ratio > 0):
        raise ValueError("ratio must be None or a finite number > 0")
    handles = [s._open() for s in sets]
    if len(pr) == 0:
        return []
    for ia, ib in pr.tolist():
        if sets[ia].dim != sets[ib].dim:
            raise ValueError(f"desc1 and desc2 differ in dimension: {sets[ia].dim} and {sets[ib].dim}")
    if len({s._ctx for s in sets}) != 1:
        raise ValueError("the DescriptorSets live on different devices")
    pr32 = np.ascontiguousarray(pr, dtype=np.uint32)
    rows = np.array([len(sets[ia]) for ia in pr[:, 0].tolist()], dtype=np.uint64)
    offsets = np.zeros(len(pr) + 1, dtype=np.uintp)
    offsets[1:] = np.cumsum(rows)
    total = int(offsets[-1])
    matches = np.empty((total, 2), dtype=np.uint32)
    ratios = np.empty(total, dtype=np.float64)
    counts = np.zeros(len(pr), dtype=np.uintp)
    hs = (C.c_void_p * len(handles))(*handles)
    N.check(N.lib.gcr_match_set_pairs(sets[0]._ctx, C.addressof(hs), len(handles), pr32.ctypes.data, len(pr),
                                      _match_options(ratio, mutual), matches.ctypes.data, ratios.ctypes.data,
                                      offsets.ctypes.data, counts.ctypes.data, None))
    out = []
    for k in range(len(pr)):
        lo, m = int(offsets[k]), int(counts[k])
        out.append((matches[lo:lo + m].astype(np.int64), ratios[lo:lo + m].copy()))
    return out


def verify_pairs(sets, pairs, kind, threshold, ratio=0.8, mutual=True, iterations=1024, seed=0, refine=False, *,
                 backend="gpu", device=None):
    """Match many pairs of images and verify every pair's geometry, each step
    one call: ``match_pairs(sets, pairs, ratio, mutual)``, then
    ``correspondences_from_matches`` per pair, then
    ``pygcransac.verify_many(rows, kind, threshold, iterations, seed=seed,
    refine=refine)`` on the pairs that have enough matches.

    ``sets`` is a sequence of ``DescriptorSet`` with keypoints, ``pairs`` a
    sequence of index pairs into it.  ``kind`` is ``"homography"`` or
    ``"fundamental"``; ``threshold`` and ``seed`` are a scalar or one value per
    pair.  ``backend="host"`` runs both steps' host twins without a GPU and
    gives the same bytes; ``sets`` are then ``(desc, keypoints)`` tuples, which
    ``backend="gpu"`` accepts as well (it uploads them for the call).

    Returns one ``(matches, ratios, record)`` per pair: ``match_pairs``'s
    arrays and ``verify_many``'s dict.  A pair with fewer matches than a
    minimal sample (4 / 7) is not sent down: its record has ``model=None``,
    an all-False mask, zero inliers, score and iterations and slot -1.  A set
    without keypoints is a ValueError."""
    from . import pygcransac as G

    if kind not in _GUIDED_KINDS:
        raise ValueError(f"kind must be 'homography' or 'fundamental', got {kind!r}")
    if backend not in ("gpu", "host"):
        raise ValueError(f"backend must be 'gpu' or 'host', got {backend!r}")
    sets = list(sets)
    pr = np.asarray(pairs)
    if pr.size == 0:
        pr = np.zeros((0, 2), dtype=np.int64)
    if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer):
        raise ValueError("pairs must be a sequence of integer pairs (ia, ib)")
    if pr.size and (pr.min() < 0 or pr.max() >= len(sets)):
        raise ValueError(f"pairs index past the {len(sets)} sets")
    tuples = [not isinstance(s, DescriptorSet) for s in sets]
    pos = []
    for k, s in enumerate(sets):
        if tuples[k]:
            if not (isinstance(s, (tuple, list)) and len(s) == 2):
                raise ValueError(f"sets[{k}] must be a DescriptorSet or a (desc, keypoints) tuple")
            if s[1] is None:
                raise ValueError(f"sets[{k}] has no keypoints")
            pos.append(_positions(s[1], f"sets[{k}] keypoints"))
        else:
            if backend == "host":
                raise ValueError("backend='host' takes (desc, keypoints) tuples: a DescriptorSet lives on the GPU")
            if not s.has_keypoints:
                raise ValueError(f"sets[{k}] has no keypoints")
            pos.append(s._positions)
    if backend == "host":
        found = [match_descriptors(sets[ia][0], sets[ib][0], ratio, mutual, backend="host") for ia, ib in pr.tolist()]
    else:
        made = [DescriptorSet(s[0], s[1], device=device) if tuples[k] else None for k, s in enumerate(sets)]
        try:
            found = match_pairs([m if m is not None else s for m, s in zip(made, sets)], pr, ratio, mutual)
        finally:
            for m in made:
                if m is not None:
                    m.close()
    need = 4 if kind == "homography" else 7
    rows = []
    for (ia, ib), (matches, _) in zip(pr.tolist(), found):
        a, b = pos[ia][matches[:, 0]], pos[ib][matches[:, 1]]
        rows.append(np.ascontiguousarray(np.column_stack([a[:, 0], a[:, 1], b[:, 0], b[:, 1]])))
    down = [k for k, r in enumerate(rows) if len(r) >= need]

    def per_pair(v):
        a = np.asarray(v)
        return a if a.ndim == 0 else a[down] if a.shape == (len(rows),) else a

    recs = G.verify_many([rows[k] for k in down], kind, per_pair(threshold), iterations, seed=per_pair(seed),
                         backend=backend, device=device, refine=refine)
    out = []
    it = iter(recs)
    for k, (matches, ratios) in enumerate(found):
        if len(rows[k]) >= need:
            rec = next(it)
        else:
            rec = {"model": None, "mask": np.zeros(len(rows[k]), dtype=bool), "inliers": 0, "score": 0.0, "slot": -1,
                   "iterations": 0}
            if refine:
                rec["refined"] = None
        out.append((matches, ratios, rec))
    return out


def fundamental_from_essential(E, K1, K2) -> np.ndarray:
    """F = K2^-T E K1^-1: the fundamental matrix of the pixel coordinates from
    an essential matrix (findEssentialMatrix, findGravityEssentialMatrix) and
    the two calibration matrices, for ``match_descriptors_guided``."""
    E, K1, K2 = (np.asarray(a, dtype=np.float64) for a in (E, K1, K2))
    if E.shape != (3, 3) or K1.shape != (3, 3) or K2.shape != (3, 3):
        raise ValueError("E, K1 and K2 must be 3 x 3")
    return np.linalg.inv(K2).T @ E @ np.linalg.inv(K1)


def correspondences_from_matches(kp1, kp2, matches, sift=False) -> np.ndarray:
    """The estimators' rows from matched keypoints.  ``kp1`` / ``kp2`` are read
    as by ``keypoints_to_array``, ``matches`` is (M, 2) rows (i, j) into them.

    Returns (M, 4) float64 rows x1, y1, x2, y2 (findHomography,
    findFundamentalMatrix, ...); with ``sift=True`` the (M, 8) rows
    findHomographySIFT takes: x1, y1, x2, y2, q1, q2, alpha1, alpha2 with the
    keypoint sizes as the lengths q and the orientations in RADIANS.  A
    matched keypoint without an angle (-1, OpenCV's convention) is then a
    ValueError."""
    a, b = keypoints_to_array(kp1), keypoints_to_array(kp2)
    m = np.asarray(matches)
    if m.ndim != 2 or m.shape[1] != 2:
        raise ValueError("matches must have shape (M, 2): rows (i, j)")
    if m.size and not np.issubdtype(m.dtype, np.integer):
        raise ValueError("matches must be an integer array")
    m = m.astype(np.int64)
    if m.size and (m.min() < 0 or m[:, 0].max() >= len(a) or m[:, 1].max() >= len(b)):
        raise ValueError("matches index past the keypoints")
    r1, r2 = a[m[:, 0]], b[m[:, 1]]
    if not sift:
        return np.ascontiguousarray(np.column_stack([r1[:, 0], r1[:, 1], r2[:, 0], r2[:, 1]]))
    bad = int(((r1[:, 3] == -1) | (r2[:, 3] == -1)).sum())
    if bad:
        raise ValueError(f"{bad} matched keypoints have no orientation (angle -1)")
    return np.ascontiguousarray(np.column_stack([r1[:, 0], r1[:, 1], r2[:, 0], r2[:, 1], r1[:, 2], r2[:, 2],
                                                 np.deg2rad(r1[:, 3]), np.deg2rad(r2[:, 3])]))
