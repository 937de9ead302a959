"""Seeded training sets for the vocabulary-training tests (test_bow_train_cpu.py,
test_gpu_bow_train.py) and their restated vocabularies, built once per process and shared."""
from __future__ import annotations

import functools

import numpy as np

import restate_bow_train as RT

N_ROWS = 5000
KL = ((2, 1), (3, 4), (10, 3), (17, 2), (64, 1))
CASES = ("random", "clustered", "duplicates", "identical", "gaps")


def split(n: int, n_images: int, rng, empty=()):
    """n rows over n_images images of uneven sizes; the images in ``empty`` hold none."""
    full = [i for i in range(n_images) if i not in empty]
    cuts = np.sort(rng.integers(0, n + 1, len(full) - 1))
    sizes = np.diff(np.concatenate([[0], cuts, [n]]))
    counts = np.zeros(n_images, np.int64)
    counts[full] = sizes
    return [int(c) for c in counts]


def flip(rows, fraction, rng):
    bits = np.unpackbits(rows, axis=1)
    return np.packbits(bits ^ (rng.random(bits.shape) < fraction).astype(np.uint8), axis=1)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (descriptors (n, 32) uint8, counts per image)."""
    if name == "random":
        rng = np.random.default_rng(1)
        return rng.integers(0, 256, (N_ROWS, 32), dtype=np.uint8), split(N_ROWS, 40, rng)
    if name == "clustered":  # noisy copies of 300 prototypes, 5 % of the bits flipped
        rng = np.random.default_rng(2)
        proto = rng.integers(0, 256, (300, 32), dtype=np.uint8)
        return flip(proto[rng.integers(0, 300, N_ROWS)], 0.05, rng), split(N_ROWS, 40, rng)
    if name == "duplicates":  # 7 distinct rows x 40, interleaved
        rng = np.random.default_rng(3)
        rows = np.repeat(rng.integers(0, 256, (7, 32), dtype=np.uint8), 40, axis=0)
        return rows[rng.permutation(280)], split(280, 9, rng)
    if name == "identical":
        rng = np.random.default_rng(4)
        return np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 150, axis=0), split(150, 5, rng)
    if name == "gaps":  # images without descriptors first, in between and last
        rng = np.random.default_rng(5)
        proto = rng.integers(0, 256, (40, 32), dtype=np.uint8)
        return flip(proto[rng.integers(0, 40, 700)], 0.08, rng), split(700, 12, rng, empty=(0, 4, 5, 11))
    raise KeyError(name)


def images(desc, counts):
    at = np.concatenate([[0], np.cumsum(counts)])
    return [desc[at[i]:at[i + 1]] for i in range(len(counts))]


@functools.lru_cache(maxsize=None)
def recursive(name: str, k: int, L: int, max_iterations: int = 100, seed: int = 0) -> RT.Trained:
    return RT.train_recursive(*case(name), k, L, max_iterations, seed)


@functools.lru_cache(maxsize=None)
def levels(name: str, k: int, L: int, max_iterations: int = 100, seed: int = 0) -> RT.Trained:
    return RT.train_levels(*case(name), k, L, max_iterations, seed)
