"""The octree gather's plan (csrc/tree.hip: k_tree_test, k_tree_scan, k_tree_fill, k_tree_offsets) against a host model with its
state (tests/tree_plan_ref.py), over scenes with exact leaf control and camera scripts (tests/tree_plan_cases.py).  No GPU:
  * the unmutated model's list equals oracle/tree_oracle.py::gather's at every step of every script, for two member permutations;
  * each of the model's ten mutations changes the list (or writes outside its arrays) at some step of the case list;
  * the case list keeps the properties the plan needs to be exercised (shared buckets at the batch edges, ties, near ties, mixed
    cull, none-then-all, scale jumps both ways, the clamp bucket) - conditions, not measurements.
The same scripts run on the device in tests/test_gpu_tree_plan.py."""
import numpy as np
import pytest

import tree_plan_cases as cases
import tree_plan_ref as ref
from gaussiansplats3d_amd import SplatTree

MUTATION_SCENES = ("lat9", "lat17", "lat257", "clusters10k")
M9_STEP = "d"                                # every leaf in one bucket: the shared bucket (m9) is judged on


def _model(name, seed, mutation=None):
    mn, mx = cases.scene_box(cases.make_scene(name)["centers"])
    return ref.PlanModel(cases.oracle_leaves(name), mn, mx, seed, mutation)


def _same(got, want):
    return got["total"] == len(want) and not got["oob"] and np.array_equal(got["list"], want)


def _print_table(name):
    print("\n%s: %d leaves, %d splats" % (name, len(cases.oracle_leaves(name)), len(cases.make_scene(name)["centers"])))
    print("  step  kept/leaves       scale  buckets  max occ  ties  near ties  clamp")
    for k, s in enumerate(cases.make_script(name)):
        r = cases.step_report(name, k)
        print("  %-4s  %5d/%-5d  %10.4g  %7d  %7d  %4d  %9d  %5d" % (s["tag"], r["kept"], r["leaves"], r["scale"], len(r["occupancy"]),
                                                                    r["max_occupancy"], r["ties"], r["near_ties"], r["clamp"]))


@pytest.mark.parametrize("name", cases.SCENES)
def test_model_equals_the_oracle_at_every_step(name):
    """Two different member permutations: the order inside a bucket's member list must not matter."""
    _print_table(name)
    want = cases.oracle_lists(name)
    for seed in (11, 12):
        model = _model(name, seed)
        for k, s in enumerate(cases.make_script(name)):
            got = model.gather(s["model_view"], s["fov"], s["width"], s["height"], s["gather_all"])
            assert not got["oob"], (name, seed, s["tag"], got["oob"][:3])
            assert got["total"] == len(want[k]), (name, seed, s["tag"])
            assert got["kept"] == cases.step_report(name, k)["kept"], (name, seed, s["tag"])
            np.testing.assert_array_equal(got["list"], want[k], err_msg="%s seed %d step %s" % (name, seed, s["tag"]))
            # the tables the next gather relies on
            assert not model.hist.any(), (name, seed, s["tag"], "hist is not zero after the gather")


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_every_mutation_is_caught(mutation):
    caught = {}
    for name in MUTATION_SCENES:
        want = cases.oracle_lists(name)
        model = _model(name, 11, mutation)
        for k, s in enumerate(cases.make_script(name)):
            got = model.gather(s["model_view"], s["fov"], s["width"], s["height"], s["gather_all"])
            if not _same(got, want[k]):
                caught.setdefault(name, []).append(s["tag"] + ("!" if got["oob"] else ""))
    print("\n%s caught at (! = writes outside its arrays): %s" % (mutation, caught))
    assert caught, "no step of the case list notices mutation " + mutation
    if mutation == "m9":
        assert any(M9_STEP in [t.rstrip("!") for t in tags] for tags in caught.values())
    if mutation == "m10":                    # only the non-affine step reaches the clamp
        assert all([t.rstrip("!") for t in tags] == ["l"] for tags in caught.values())


def _reports():
    return {name: [cases.step_report(name, k) for k in range(len(cases.make_script(name)))] for name in cases.SCENES}


def test_case_list_keeps_its_properties():
    reps = _reports()
    every = [r for rs in reps.values() for r in rs]
    occupancies = set(o for r in every for o in r["occupancy"].values())
    assert {1, 2, 8, 9, 16, 17} <= occupancies, sorted(occupancies)[:40]
    assert max(occupancies) >= 512
    assert any(r["ties"] >= 100 for r in every)
    assert any(r["near_ties"] >= 30 for r in every)
    assert any(0.2 * r["leaves"] <= r["kept"] <= 0.8 * r["leaves"] for r in every)
    assert any(r["clamp"] >= 9 for r in every)
    for name, rs in reps.items():
        tags = [s["tag"] for s in cases.make_script(name)]
        assert rs[tags.index("i")]["kept"] == 0 and rs[tags.index("j")]["kept"] == rs[tags.index("j")]["leaves"] > 0
        assert tags.index("j") == tags.index("i") + 1
        ratios = [rs[k + 1]["scale"] / rs[k]["scale"] for k in range(len(rs) - 1)]
        assert max(ratios) > 1e6 and min(ratios) < 1e-6, (name, ratios)
        h = rs[tags.index("h")]
        assert h["occupancy"].get(0, 0) >= 1, "the eye sits on a leaf centre: distance 0, bucket 0"
    assert reps["lat1"][[s["tag"] for s in cases.make_script("lat1")].index("h")]["scale"] == 1.0       # far == 0
    # (m9) every shared bucket of the step it is judged on holds leaves of different splat counts
    for name in MUTATION_SCENES:
        tags = [s["tag"] for s in cases.make_script(name)]
        r = reps[name][tags.index(M9_STEP)]
        shared = [m for m in r["members"].values() if len(m) >= 2]
        assert shared and r["max_occupancy"] == r["leaves"]
        for m in shared:
            assert len(set(len(cases.oracle_leaves(name)[i]["indexes"]) for i in m)) >= 2


@pytest.mark.parametrize("name", list(cases.LATTICES))
def test_lattice_scenes_have_exactly_their_leaves(name):
    """The leaf count of every lattice scene equals its K, through the oracle builder and the host-only native builder; the leaves
    are the chosen cells (depth log2(G), the cell centres)."""
    scene = cases.make_scene(name)
    G, K = cases.LATTICES[name]
    leaves = cases.oracle_leaves(name)
    assert len(leaves) == K == scene["leaves_expected"]
    tree = SplatTree(None, scene["max_depth"], scene["max_centers"]).process_splat_mesh(scene["centers"])
    try:
        assert tree.info().leaves == K
        bounds, centers, depths, offsets, indexes = tree.leaves()
    finally:
        tree.dispose()
    np.testing.assert_array_equal(centers, np.array([lf["center"] for lf in leaves]).reshape(-1, 3))
    np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), [len(lf["indexes"]) for lf in leaves])
    np.testing.assert_array_equal(indexes, np.concatenate([lf["indexes"] for lf in leaves]))
    if K > 1:
        assert set(depths.tolist()) == {scene["max_depth"] + 1}
        cell = 8.0 / G
        assert np.all(np.mod(centers + 4.0, cell) == cell / 2), "leaf centres are the cell centres"
        assert len(scene["centers"]) < 6000
