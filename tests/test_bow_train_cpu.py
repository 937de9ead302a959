"""CPU checks of the restated vocabulary training (tests/restate_bow_train.py): the literal recursion
and the level-synchronous form the kernels follow agree byte for byte, and the trees have the shape
lislam_bow_create and restate_bow.Vocabulary expect."""
import numpy as np
import pytest

import bow_train_cases as TC
import restate_bow as RB
import restate_bow_train as RT

GRID = [(name, k, L) for name in TC.CASES for (k, L) in TC.KL]


def _same(a: RT.Trained, b: RT.Trained):
    return (a.parent.tobytes() == b.parent.tobytes() and a.descriptor.tobytes() == b.descriptor.tobytes()
            and a.weight.tobytes() == b.weight.tobytes() and np.array_equal(a.leaf_of, b.leaf_of) and a.stats == b.stats
            and a.events == b.events)


def test_generator_constants():
    """splitmix64 as published (Steele, Lea, Flood 2014; Vigna's splitmix64.c): the first outputs of a
    generator seeded with 1234567."""
    assert RT.splitmix64(1234567) == 6457827717110365317
    assert RT.splitmix64((1234567 + RT.GOLDEN) & RT.MASK) == 3203168211198807973
    assert RT.reduce(RT.MASK, 10) == 9 and RT.reduce(0, 10) == 0 and RT.reduce(1 << 63, 7) == 3


@pytest.mark.parametrize("name,k,L", GRID)
def test_two_forms_agree_and_the_tree_is_well_formed(name, k, L):
    rec, lev = TC.recursive(name, k, L), TC.levels(name, k, L)
    assert _same(rec, lev)
    desc, counts = TC.case(name)
    n = rec.parent.shape[0]
    assert rec.parent[0] == -1 and np.all(rec.parent[1:] < np.arange(1, n)) and np.all(rec.parent[1:] >= 0)
    voc = RB.Vocabulary(rec.parent, rec.descriptor, rec.weight)
    for kids in voc.children:  # consecutive, in slot order
        assert len(kids) <= k and kids == list(range(kids[0], kids[0] + len(kids))) if kids else True
    assert sum(rec.stats["level_capped"]) == 0  # max_iterations = 100 leaves these inputs uncapped
    assert max(rec.stats["level_iterations"]) < 100
    assert np.all(rec.weight[[i for i in range(n) if voc.children[i]]] == 0)
    assert np.all(np.isfinite(rec.weight)) and np.all(rec.weight >= 0)
    # a converged run: the descent ends in the leaf training left the descriptor in, or, among the
    # children of a <= k node, in the first copy of a duplicate
    words, _ = voc.transform(desc)
    leaf = voc.leaf_node[words]
    moved = np.nonzero(leaf != rec.leaf_of)[0]
    for i in moved:
        assert rec.parent[leaf[i]] == rec.parent[rec.leaf_of[i]] and leaf[i] < rec.leaf_of[i]
        assert rec.descriptor[leaf[i]].tobytes() == desc[i].tobytes() == rec.descriptor[rec.leaf_of[i]].tobytes()
    if name in ("random", "clustered"):
        assert moved.shape[0] == 0


def test_rules_of_ours_are_met():
    assert max(TC.recursive("clustered", k, L).events["empty_cluster"] for k, L in TC.KL) >= 1
    assert all(TC.recursive("duplicates", k, L).events["s_zero"] >= 1 for k, L in ((10, 3), (17, 2), (64, 1)))
    # 7 distinct rows: no node gets more than 7 children, whatever k
    rec = TC.recursive("duplicates", 10, 3)
    assert np.bincount(rec.parent[1:]).max() == 7
    # identical rows: one child holds them all, level after level, down to L
    rec = TC.recursive("identical", 3, 4)
    assert rec.parent.tolist() == [-1, 0, 1, 2, 3] and rec.stats["level_iterations"] == [2, 2, 2, 2]


@pytest.mark.parametrize("cap", [1, 2])
def test_the_iteration_cap(cap):
    rec, lev = TC.recursive("random", 10, 3, cap), TC.levels("random", 10, 3, cap)
    assert _same(rec, lev)
    assert rec.stats["level_iterations"] == [cap] * 3
    if cap == 1:  # no second assignment to compare with: every clustered node stops at the cap
        assert rec.stats["level_capped"] == rec.stats["level_clustered"]
    else:  # a node whose second assignment equals the seeding's has converged, not stopped
        assert rec.stats["level_capped"][:2] == rec.stats["level_clustered"][:2] == [1, 10]
        assert 0 < rec.stats["level_capped"][2] <= rec.stats["level_clustered"][2]
    assert rec.descriptor.tobytes() != TC.recursive("random", 10, 3).descriptor.tobytes()


def test_empty_input_and_image_count():
    root = RT.train_recursive(np.zeros((0, 32), np.uint8), [0, 0], 10, 5)
    assert root.parent.tolist() == [-1] and root.weight.tolist() == [0.0]
    assert _same(root, RT.train_levels(np.zeros((0, 32), np.uint8), [0, 0], 10, 5))
    desc, counts = TC.case("gaps")
    a = RT.train_recursive(desc, counts, 3, 4)
    b = RT.train_recursive(desc, counts + [0], 3, 4)  # one more empty image: N changes, the tree does not
    assert a.parent.tobytes() == b.parent.tobytes() and a.descriptor.tobytes() == b.descriptor.tobytes()
    leaves = a.weight > 0
    assert leaves.any() and np.all(b.weight[leaves] > a.weight[leaves])


def test_seeds_differ():
    assert TC.recursive("random", 10, 3, 100, 1).descriptor.tobytes() != TC.recursive("random", 10, 3).descriptor.tobytes()
