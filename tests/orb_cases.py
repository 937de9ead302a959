"""Inputs of the ORB edge tests (test_orb_cases_cpu.py, test_gpu_orb_edges.py): images at the sensor's
other shapes and at shapes whose upper pyramid levels shrink to a few pixels, images that tie every
FAST score or Harris response, budgets that empty whole levels, masks and cloud tracks that filter
keypoints, images that carry a level past the library's room (`lcap`), descriptor sets at the
matcher's tile edges, and small frame sequences for the tracker and the batch.  Deterministic, numpy
only; `oracle` and `synth` are passed in by the tests where a case is cut from the oracle's own output.

A detect case is (name, image (H, W) u8, cloud_track (H, W, 4) f32, mask (H, W) u8 or None, nfeatures)."""
from __future__ import annotations

import math

import numpy as np

LEVELS = 8

SHAPES = ((16, 512), (32, 1024), (32, 2048), (128, 1024), (24, 100), (17, 67), (8, 1024), (9, 9), (8, 8))
MASKED_SHAPES = ((16, 512), (128, 1024), (17, 67))
ODD_WIDTH = (24, 102)  # W % 4 == 2: the aligned dword fetches of the Harris / angle patches straddle rows' ends
MATCH_SIZES = ((1, 1), (1, 300), (300, 1), (15, 17), (16, 16), (17, 15), (255, 257), (256, 256), (257, 255), (513, 64),
               (0, 5), (5, 0))
BUDGETS = (1, 7, 16384)
BUDGET_NPER = {1: [0, 0, 0, 0, 0, 0, 0, 1], 7: [2, 1, 1, 1, 1, 1, 1, 0]}
CAPACITY_CASES = ("capacity_tile16_n100", "capacity_tile8_n200")
EMPTY_CASES = ("content_zeros", "content_255")
# worked out from engine_detect_slots' `fused` condition (takes_fused_path restates it)
FUSED_SHAPES = ((16, 512), (32, 1024), (32, 2048), (24, 100), (8, 1024), (8, 8), (64, 1024))
UNFUSED_SHAPES = ((128, 1024), (17, 67), (9, 9), (24, 102))


# ------------------------------------------------------------------ the library's per-level budget, restated
def features_per_level(nfeatures: int) -> list[int]:
    """nfeaturesPerLevel of computeKeyPoints (orb.cpp) for scaleFactor 1.2f, 8 levels: float arithmetic,
    cvRound (half to even)."""
    f32 = np.float32
    factor = f32(1.0 / float(f32(1.2)))
    nd = f32(nfeatures) * (f32(1) - factor) / (f32(1) - f32(math.pow(float(factor), LEVELS)))
    out, total = [], 0
    for _ in range(LEVELS - 1):
        out.append(int(np.rint(nd)))
        total += out[-1]
        nd = f32(nd * factor)
    out.append(max(nfeatures - total, 0))
    return out


def lcap(nfeatures: int) -> list[int]:
    """Keypoints a level has room for in the library (engine_init): 2 * n_l + 64.  The reference's
    retainBest keeps every response tied with the n_l-th and has no such bound."""
    return [2 * n + 64 for n in features_per_level(nfeatures)]


def level_sizes(H: int, W: int) -> list[tuple[int, int]]:
    """(w, h) of the 8 pyramid levels (engine_init: cvRound(size / 1.2f^l) in float)."""
    out = []
    for l in range(LEVELS):
        inv = np.float32(1.0) / np.float32(math.pow(float(np.float32(1.2)), l))
        out.append((int(np.rint(np.float32(W) * inv)), int(np.rint(np.float32(H) * inv))))
    return out


def takes_fused_path(H: int, W: int) -> bool:
    """engine_detect_slots' `fused`: the one-workgroup-per-scan k_orb_pyramid + k_orb_roiblur path
    (else k_orb_level per level + k_orb_blur).  Dword rows, level 1 at most 64 rows, a level-0 padded row
    of at most 1024 dwords, level 0 within 64 KiB of LDS, level 1 within 48 KiB, level 2 within 32 KiB."""
    lv = level_sizes(H, W)
    stride0 = (W + 2 * 23 + 15) & ~15
    return (W % 4 == 0 and lv[1][1] <= 64 and stride0 // 4 <= 1024 and ((W * H + 15) & ~15) <= 64 * 1024
            and lv[1][0] * lv[1][1] <= 48 * 1024 and lv[2][0] * lv[2][1] <= 32 * 1024)


def level_counts(kp) -> list[int]:
    """Keypoints per octave of an (n, 6) keypoint array."""
    return [int(np.sum(kp[:, 5] == l)) for l in range(LEVELS)]


# ------------------------------------------------------------------ the cross-check matcher in numpy
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint16)


def hamming(a, b) -> np.ndarray:
    """(len(a), len(b)) Hamming distances of 32-byte descriptors."""
    a, b = np.asarray(a, np.uint8).reshape(-1, 32), np.asarray(b, np.uint8).reshape(-1, 32)
    D = np.zeros((a.shape[0], b.shape[0]), np.int64)
    for i0 in range(0, a.shape[0], 8):  # a few query rows at a time: 65535 trains stay within memory
        D[i0:i0 + 8] = _POP[a[i0:i0 + 8, None, :] ^ b[None, :, :]].sum(2)
    return D


def crosscheck_match(a, b) -> np.ndarray:
    """BFMatcher(NORM_HAMMING, crossCheck = true).match(a, b) by brute force: (m, 3) = query, train,
    distance in query order.  Each train row takes its first nearest query; a query keeps the nearest
    of the trains that took it, the first among equals."""
    D = hamming(a, b)
    if D.shape[0] == 0 or D.shape[1] == 0:
        return np.zeros((0, 3), np.int64)
    tbest = D.argmin(0)  # per train the first nearest query
    best = {}
    for i in range(D.shape[1]):
        j, d = int(tbest[i]), int(D[tbest[i], i])
        if j not in best or d < best[j][1]:
            best[j] = (i, d)
    return np.array([[j, best[j][0], best[j][1]] for j in sorted(best)], np.int64).reshape(-1, 3)


# ------------------------------------------------------------------ images, tracks, masks
def hand_held_mask(H, W, crop=3):
    m = np.full((H, W), 255, np.uint8)
    j = np.arange(W)
    m[:, (j < crop) | (j > W - crop)] = 0
    return m


def noise(H, W, seed=11) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def noise_blobs(H, W, seed=12) -> np.ndarray:
    """Uniform noise with a few smooth bright and dark blobs (corners at every pyramid level)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W)).astype(np.float64)
    y, x = np.mgrid[0:H, 0:W]
    for k in range(4):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        r = rng.uniform(1.5, max(2.0, min(H, W) / 3))
        img += (200.0 if k % 2 else -200.0) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def tiled(t, H=64, W=1024, seed=21) -> np.ndarray:
    """A random t x t tile repeated over the image: every response occurs once per tile, so
    retainBest's ties keep whole groups of keypoints."""
    tile = np.random.default_rng(seed).integers(0, 256, (t, t), dtype=np.uint8)
    return np.tile(tile, (H // t, W // t))


def checkerboard(H=64, W=1024, px=4) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    return (((y // px + x // px) % 2) * 255).astype(np.uint8)


def blocks(H=64, W=1024, px=8, seed=22) -> np.ndarray:
    b = np.random.default_rng(seed).integers(0, 2, (H // px, W // px), dtype=np.uint8) * 255
    return np.kron(b, np.ones((px, px), np.uint8))


def frame_image(H=64, W=1024, border=6, seed=37) -> np.ndarray:
    """Flat 128 except a noisy frame `border` pixels wide along all four edges."""
    img = np.full((H, W), 128, np.uint8)
    n = noise(H, W, seed)
    edge = np.zeros((H, W), bool)
    edge[:border] = edge[-border:] = True
    edge[:, :border] = edge[:, -border:] = True
    img[edge] = n[edge]
    return img


def random_track(H, W, seed=31) -> np.ndarray:
    """Every point well away from zero on every axis: no keypoint is filtered."""
    rng = np.random.default_rng(seed)
    t = np.zeros((H, W, 4), np.float32)
    t[..., :3] = rng.uniform(0.5, 30.0, (H, W, 3)) * rng.choice([-1.0, 1.0], (H, W, 3))
    t[..., 3] = rng.uniform(0, 255, (H, W))
    return t


def keypoint_pixels(kp, W) -> np.ndarray:
    """Flat level-0 pixel of each keypoint, as the cloud_track lookup rounds it."""
    return np.rint(kp[:, 1]).astype(int) * W + np.rint(kp[:, 0]).astype(int)


# ------------------------------------------------------------------ detect cases
TINY_SEEDS = {(9, 9): 106, (8, 8): 104}  # most 8 x 8 and 9 x 9 images have no corner at all: seeds that give >= 2


def shape_image(H, W):
    return noise_blobs(H, W, TINY_SEEDS.get((H, W), 100 + H + W))


def shape_cases():
    out = []
    for H, W in SHAPES + (ODD_WIDTH,):
        out.append((f"shape_{H}x{W}", shape_image(H, W), random_track(H, W, H * W), None, 500))
    for H, W in MASKED_SHAPES:
        out.append((f"shape_{H}x{W}_masked", shape_image(H, W), random_track(H, W, H * W), hand_held_mask(H, W), 500))
    return out


def content_cases():
    tr = random_track(64, 1024)
    return [("content_zeros", np.zeros((64, 1024), np.uint8), tr, None, 1000),
            ("content_255", np.full((64, 1024), 255, np.uint8), tr, None, 1000),
            ("content_checker4", checkerboard(), tr, None, 1000),
            ("content_blocks8", blocks(), tr, None, 1000),
            ("content_noise", noise(64, 1024), tr, None, 1000),
            ("content_frame", frame_image(), tr, None, 1000),
            ("content_tied", tiled(16), tr, None, 1000)]


def budget_cases():
    tr = random_track(64, 1024)
    return [(f"budget_{n}", noise(64, 1024), tr, None, n) for n in BUDGETS]


def mask_cases(oracle):
    img, tr = noise(64, 1024), random_track(64, 1024)
    kp, _, _ = oracle.orb_detect(img, tr, 1000, None)
    one = np.zeros((64, 1024), np.uint8)
    lv0 = kp[kp[:, 5] == 0]
    k = lv0[len(lv0) // 2]  # a level-0 keypoint: its own pixel decides
    one[int(k[1]), int(k[0])] = 255
    odd = np.random.default_rng(41).integers(0, 4, (64, 1024)).astype(np.uint8)  # 0 masks; 1, 2, 3 do not
    return [("mask_zero", img, tr, np.zeros((64, 1024), np.uint8), 1000),
            ("mask_one_pixel", img, tr, one, 1000),
            ("mask_not_255", img, tr, odd, 1000)]


def track_case(oracle):
    """The noise image with x, y, z, or all three zero under disjoint thirds of the oracle's
    keypoints: the feature tracker's filter drops the x and the all thirds, mapOptimization's only the
    all third.  Returns the case; run it with map_filter False and True."""
    img, tr = noise(64, 1024), random_track(64, 1024).reshape(-1, 4)
    kp, _, _ = oracle.orb_detect(img, tr, 1000, None)
    pix = np.unique(keypoint_pixels(kp, 1024))
    tr[pix[0::4], 0] = 0.0
    tr[pix[1::4], 1] = 0.0
    tr[pix[2::4], 2] = 0.0
    tr[pix[3::4], :3] = (0.009, -0.009, 0.0)
    return ("track_zero_axes", img, tr.reshape(64, 1024, 4), None, 1000)


def map_filter_keep(track) -> np.ndarray:
    """mapOptimization's zero filter (mapOptimization.cpp:620): dropped only when |x|, |y| and |z| are
    all below 0.01 (floats compared with the double 0.01)."""
    t = np.asarray(track, np.float32).reshape(-1, 4).astype(np.float64)
    return ~((np.abs(t[:, 0]) < 0.01) & (np.abs(t[:, 1]) < 0.01) & (np.abs(t[:, 2]) < 0.01))


def map_filter_reference(oracle, img, track, nfeatures, mask):
    """What lislam_orb_detect_map must return, from oracle.orb_detect (which filters on |x| alone): the
    oracle on a track whose x is 1 wherever the three-axis test keeps the point, the points gathered from
    the track itself."""
    t = np.array(track, np.float32).reshape(-1, 4)
    t2 = t.copy()
    t2[map_filter_keep(t), 0] = 1.0
    kp, de, _ = oracle.orb_detect(img, t2, nfeatures, mask)
    return kp, de, t[keypoint_pixels(kp, img.shape[1]), :3]


def capacity_cases():
    tr = random_track(64, 1024)
    return [("capacity_tile16_n100", tiled(16), tr, None, 100),
            ("capacity_tile8_n200", tiled(8, seed=24), tr, None, 200)]


def detect_cases(oracle):
    """Every case lislam_orb_detect must reproduce bit for bit (the capacity cases are apart)."""
    return shape_cases() + content_cases() + budget_cases() + mask_cases(oracle) + [track_case(oracle)]


# the names detect_cases builds, in order (for parametrized tests; test_orb_cases_cpu.py holds the two equal)
DETECT_NAMES = tuple([f"shape_{H}x{W}" for H, W in SHAPES + (ODD_WIDTH,)] + [f"shape_{H}x{W}_masked" for H, W in MASKED_SHAPES] +
                     ["content_zeros", "content_255", "content_checker4", "content_blocks8", "content_noise", "content_frame",
                      "content_tied"] + [f"budget_{n}" for n in BUDGETS] + ["mask_zero", "mask_one_pixel", "mask_not_255"] +
                     ["track_zero_axes"])
MATCH_NAMES = tuple([f"sizes_{q}x{t}" for q, t in MATCH_SIZES] + ["identical_rows", "zeros_vs_ones", "permuted", "low_bytes",
                                                                  "train_65535"])


# ------------------------------------------------------------------ match cases
def random_desc(rng, n) -> np.ndarray:
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def match_cases():
    """(name, query descriptors, train descriptors)."""
    rng = np.random.default_rng(51)
    out = [(f"sizes_{nq}x{nt}", random_desc(rng, nq), random_desc(rng, nt)) for nq, nt in MATCH_SIZES]
    row = random_desc(rng, 1)
    out.append(("identical_rows", np.repeat(row, 40, 0), np.repeat(row, 50, 0)))
    out.append(("zeros_vs_ones", np.zeros((33, 32), np.uint8), np.full((47, 32), 255, np.uint8)))  # every distance 256
    a = random_desc(rng, 200)
    out.append(("permuted", a, a[rng.permutation(200)]))
    lo = np.zeros((300, 32), np.uint8)
    lo[:, :2] = rng.integers(0, 256, (300, 2))
    lo2 = np.zeros((310, 32), np.uint8)
    lo2[:, :2] = rng.integers(0, 256, (310, 2))
    out.append(("low_bytes", lo, lo2))  # distances <= 16: heavy ties
    a = random_desc(rng, 64)
    b = random_desc(rng, 65535)
    b[-1] = a[0]
    b[40000] = a[1]
    out.append(("train_65535", a, b))  # train indices beyond 32767 in the packed (distance << 16) | train
    return out


# ------------------------------------------------------------------ small-shape sequences (tracker, batch)
SEQ_H, SEQ_W, SEQ_NFEATURES = 16, 512, 500


def scan_of(synth, image, index=3):
    """An organized (H, W, 4) scan whose a1 intensity image is `image`: a synthetic scan's geometry
    (the same for every frame, so a repeated image is a repeated frame) with the image as its
    intensity channel."""
    H, W = image.shape
    scan = np.array(synth.make_scan(index, H, W), np.float32)
    scan[..., 3] = image.astype(np.float32)
    return scan


def shifted(img, dx):
    return np.roll(img, dx, axis=1)


def small_sequence_images():
    """Four 16 x 512 frames: the blob-noise image moving by a few columns, the second frame repeated
    (equal keypoint counts: the good-frame test fails and both frames re-detect with 2n)."""
    base = noise_blobs(SEQ_H, SEQ_W, 61)
    return [base, shifted(base, 2), shifted(base, 2), shifted(base, 5)]


def few_matches_images():
    """Two 16 x 512 frames with a handful of keypoints each (a six-column crop of the "frame" image on
    flat 128, moved by one column), so that fewer than 4 matches are selected and the G >= 4 rule fails
    the pair."""
    f = frame_image(SEQ_H, SEQ_W, 6, 63)
    a = np.full((SEQ_H, SEQ_W), 128, np.uint8)
    a[:, 100:106] = f[:, :6]
    b = np.full((SEQ_H, SEQ_W), 128, np.uint8)
    b[:, 101:107] = f[:, :6]
    return [a, b]


def small_sequence(synth):
    """(images, scans) of the small-shape tracker / batch test: the moving frames, then the
    few-matches pair."""
    imgs = small_sequence_images() + few_matches_images()
    return imgs, np.stack([scan_of(synth, im) for im in imgs])
