"""The relations of tests/metamorphic.py belong to the ops, not to the kernels: every (op, family) pair the table marks as holding
is asserted here on the op's reference callable (the *_ref.py restatements) at small sizes, every exclusion is proven by a
counterexample on which the relation fails on the reference, the table keeps its conditions, the helpers are checked against
brute force, four deliberately broken ops are caught by the family meant to catch them (the precedent of
test_kernel_bounds_cpu.py), and the placement plan of family T meets its seam conditions.  No GPU needed."""
import re

import numpy as np
import pytest

import instances_ref
import measure_ref
import metamorphic as mm
import shape_ref

SMALL_CANVAS = (24, 28)
SMALL_PLAN = [(0, 0), (1, 0), (0, 3), (5, 7), (8, 10), (7, 2)]           # (8, 10) ends in the last row and the last column
SMALL_VIEWS = (1, 2, 4, 5, 7)


def small_scene(seed=1, H=16, W=18):
    """Inputs of a 16 x 18 scene with a margin of 2: a handful of cells, touching ones, a hole, ids with a gap."""
    gt, pred = instances_ref.cells_case(seed, 5, H, W, stride=2)
    gt[H // 2 - 1:H // 2 + 2, 6:12], gt[H // 2, 8] = 3, 0
    frame = np.ones((H, W), bool)
    frame[2:-2, 2:-2] = False
    gt[frame], pred[frame] = 0, 0
    assert mm.margin(gt) >= 2 and mm.margin(pred) >= 2 and len(np.unique(gt)) >= 4
    return mm.inputs_of(gt, pred)


def hand_scene():
    """Inputs of a 16 x 18 scene with a margin of 2, ids with gaps: two touching cells (2, 4), a cell with a hole (6), a pair in
    diagonal contact only (8, 10), a one-pixel cell (12) and a cell with two corners cut (14); pred is the labelling of the cells
    moved by (1, 1)."""
    g = np.zeros((16, 18), np.int32)
    g[2:7, 2:5], g[2:7, 5:9], g[2:8, 10:15], g[4:6, 12] = 2, 4, 6, 0
    g[9:11, 2:5], g[11:13, 5:8], g[9, 9], g[9:13, 10:15], g[9, 10], g[12, 14] = 8, 10, 12, 14, 0, 0
    moved = np.zeros_like(g)
    moved[1:, 1:] = g[:-1, :-1]
    pred = instances_ref.label(moved)[0]
    assert mm.margin(g) >= 2 and mm.margin(pred) >= 2
    return mm.inputs_of(g, pred)


@pytest.fixture(scope="module")
def scene():
    return hand_scene()


# ---- the helpers ----------------------------------------------------------------------------------------------------------

def test_views_form_the_dihedral_group():
    a = np.arange(15).reshape(3, 5)
    distinct = {mm.view(a, v).tobytes() + bytes(mm.view(a, v).shape) for v in mm.VIEWS}
    assert len(distinct) == 8
    for v in mm.VIEWS:
        assert np.array_equal(mm.unview(mm.view(a, v), v), a)
        assert sorted(mm.compose(v, w) for w in mm.VIEWS) == list(mm.VIEWS)            # a row of the group table is a permutation
        assert any(mm.compose(v, w) == 0 for w in mm.VIEWS)
        for w in mm.VIEWS:
            assert np.array_equal(mm.view(mm.view(a, v), w), mm.view(a, mm.compose(v, w)))
    batch = np.arange(30).reshape(2, 3, 5)
    assert np.array_equal(mm.view(batch, 5)[1], mm.view(batch[1], 5))


def test_embed_and_extract_round_trip():
    s = np.arange(1, 13).reshape(1, 3, 4)
    for dy, dx in ((0, 0), (2, 3), (4, 5)):
        e = mm.embed(s, 7, 9, dy, dx)
        assert e.shape == (1, 7, 9) and e.sum() == s.sum() and np.array_equal(mm.extract(e, 3, 4, dy, dx), s)
    assert mm.embed(s, 7, 9, 1, 1, fill=-1)[0, 0, 0] == -1
    with pytest.raises(AssertionError):
        mm.embed(s, 7, 9, 5, 0)


def test_canon_labels():
    rs = np.random.RandomState(0)
    lab = rs.randint(0, 6, (3, 7, 9))
    c = mm.canon_labels(lab)
    assert np.array_equal(mm.canon_labels(c), c) and np.array_equal(c == 0, lab == 0)
    renamed = mm.relabel(lab, lambda i: np.where(i > 0, (i * 7) % 11 + 20, 0))
    assert np.array_equal(mm.canon_labels(renamed), c)
    for img in c:
        first = [np.flatnonzero(img.ravel() == k)[0] for k in range(1, img.max() + 1)]
        assert first == sorted(first)
    assert not np.array_equal(mm.canon_labels(np.array([[1, 1, 2]])), mm.canon_labels(np.array([[1, 2, 2]])))


def test_moment_box_and_point_transport_against_brute_force():
    rs = np.random.RandomState(3)
    lab = rs.randint(0, 4, (1, 6, 9)).astype(np.int32)
    base = measure_ref.sums_batch(lab)
    for tr in [mm.Tr(v=v, shape=mm.view(lab, v).shape[-2:]) for v in mm.VIEWS[1:]] + \
              [mm.Tr(shape=(11, 15), shift=s, scene=(6, 9)) for s in ((0, 0), (5, 6), (2, 1))]:
        got = measure_ref.sums_batch(tr.apply({"ids": lab})["ids"])
        rows = slice(1, None) if tr.kind == "shift" else slice(None)
        assert np.array_equal(tr.moments(got["moments"], got["area"])[:, rows], base["moments"][:, rows])
        assert np.array_equal(tr.boxes(got["bbox"])[:, rows], base["bbox"][:, rows])
    tr = mm.Tr(v=6, shape=(9, 6))
    ys, xs = np.nonzero(mm.view(lab[0], 6) == 2)
    y, x = tr.points(ys, xs)
    assert sorted(zip(y.tolist(), x.tolist())) == sorted(zip(*(c.tolist() for c in np.nonzero(lab[0] == 2))))


def test_relabel_and_its_way_back():
    lab = np.array([[0, 1, 4], [9, 4, 0]], np.int32)
    for f in (mm.order_map, mm.top_map(9), mm.gap_permutation(np.array([1, 4, 9]), 1)):
        tr = mm.Tr(f=f, ids=lab)
        new = tr.apply({"ids": lab}, ("ids",))["ids"]
        assert np.array_equal(new == 0, lab == 0) and np.array_equal(tr.ids(new), lab)
    assert mm.relabel(lab, mm.top_map(9)).max() == (1 << 24) - 1
    assert {1, 7, 8, 500} <= set(mm.gap_permutation(np.arange(1, 9))(np.arange(1, 9)).tolist())


# ---- the table --------------------------------------------------------------------------------------------------------------

def test_table_conditions():
    excluded = [(n, f) for n, op in mm.OPS.items() for f, s in op.families.items() if s != mm.HOLDS]
    partly = [(n, f) for n, op in mm.OPS.items() for f in op.omits]                     # a family that leaves a field out counts too
    assert len(set(excluded + partly)) <= 4
    for n, f in partly:
        assert mm.OPS[n].families[f] == mm.HOLDS and mm.OPS[n].omits[f]
        assert all(e.counterexample in mm.COUNTER and e.reason for e in mm.OPS[n].omits[f].values())
    for name, op in mm.OPS.items():
        fam = mm.families(name)
        assert "B" in fam, name
        assert fam & {"D", "T"}, name
        assert len(fam) >= 3, name
        assert ("R" in op.families) == bool(op.relabel) == bool(op.id_inputs), name
    for n, f in excluded:
        assert mm.OPS[n].families[f].counterexample in mm.COUNTER and mm.OPS[n].families[f].reason
    assert all(n in mm.OPS for _, names in mm.FIXED.values() for n in names)


SAYS = {"D": r"view \d", "T": r"scene at", "R": r"ids renamed"}              # how the relation of a family names the case that failed


def test_every_exclusion_fails_on_the_reference():
    """An exclusion without a counterexample on which the reference itself breaks the relation is an error: the failure must be
    the relation's own (its message), not a stray assert."""
    for name, op in mm.OPS.items():
        for family, state in op.families.items():
            if state != mm.HOLDS:
                with pytest.raises(AssertionError, match="%s, %s.*differs" % (re.escape(name), SAYS[family])):
                    mm.COUNTER[state.counterexample](name, "ref")


def test_every_omitted_field_fails_on_the_reference_and_nothing_else_does():
    """A field that a family does not carry breaks that family's relation on the reference, on a named scene, compared alone
    with everything the family does carry; and with the omission in force the same scene passes."""
    n = 0
    for name, op in mm.OPS.items():
        for family, fields in op.omits.items():
            for field, state in fields.items():
                with pytest.raises(AssertionError, match="%s, %s.*%s differs" % (re.escape(name), SAYS[family], re.escape(repr(field)))):
                    mm.COUNTER[state.counterexample](name, "ref", field)
                mm.COUNTER[state.counterexample](name, "ref", None)
                n += 1
    assert n == 7


def test_a_normal_form_may_not_drop_a_field_it_did_not_declare():
    whole = mm.run("seg_measure", hand_scene(), "ref")
    less = {k: v for k, v in whole.items() if k != "per_image"}
    for family in "DTBR":                                               # R omits per_image from the comparison, not from the normal form
        with pytest.raises(AssertionError, match="fields"):
            mm._demand("seg_measure", family, "a dropped field", less, whole)
    mm._demand("seg_measure", "R", "declared", dict(whole, per_image=whole["per_image"] + 1), whole)
    with pytest.raises(AssertionError, match="'per_image' differs"):
        mm._demand("seg_measure", "D", "not declared for D", dict(whole, per_image=whole["per_image"] + 1), whole)


# ---- every pair that holds, on the reference ------------------------------------------------------------------------------

def holding(family):
    return [n for n, op in mm.OPS.items() if op.families.get(family) == mm.HOLDS]


@pytest.mark.parametrize("name", holding("D"))
def test_D_on_the_reference(name, scene):
    assert mm.relation_D(name, scene, "ref", SMALL_VIEWS) == len(SMALL_VIEWS)
    tall = small_scene(2, 7, 19)
    mm.relation_D(name, tall, "ref", (3, 6))


@pytest.mark.parametrize("name", holding("T"))
def test_T_on_the_reference(name, scene):
    k = mm.OPS[name].lattice
    plan = list(dict.fromkeys((dy - dy % k, dx - dx % k) for dy, dx in SMALL_PLAN))
    assert mm.relation_T(name, scene, "ref", SMALL_CANVAS, plan) == len(plan) - 1 >= 3


def test_a_lattice_is_needed_where_it_is_used():
    """An op that is held to T on a lattice only breaks T off the lattice, on the reference: the lattice hides no kernel."""
    for name, op in mm.OPS.items():
        if op.lattice > 1:
            x = mm.warp_counterexample()
            mm.relation_T(name, x, "ref", (12, 12), [(0, 0), (2, 0), (0, 2), (4, 2)])
            for odd in ((1, 0), (0, 1)):
                with pytest.raises(AssertionError, match="scene at"):
                    mm.relation_T(name, x, "ref", (12, 12), [(0, 0), odd])


@pytest.mark.parametrize("name", holding("B"))
def test_B_on_the_reference(name, scene):
    assert mm.relation_B(name, scene, "ref") == 9


@pytest.mark.parametrize("name", holding("R"))
def test_R_on_the_reference(name, scene):
    for f in mm.renamings(name, scene):
        mm.relation_R(name, scene, "ref", f)


@pytest.mark.parametrize("name", list(mm.FIXED))
def test_F_on_the_reference(name, scene):
    mm.FIXED[name][0](lambda op, x, **kw: mm.run(op, x, "ref", **kw), scene)


TIE_OPS = ("grow_cells", "split_cells[4]", "split_cells[8]", "watershed[4]", "link_frames")


@pytest.mark.parametrize("name", TIE_OPS)
def test_the_tie_rules_hold_on_the_scene_made_of_ties(name):
    """rand_ref.tie_maps puts pixels equally far from two or four ids: where a tie rule named a position, a view would show it."""
    (x,) = [x for n, x in mm.reused_scenes() if n.startswith("ties")]
    mm.relation_D(name, x, "ref", (2, 4, 7))
    mm.relation_R(name, x, "ref", mm.order_map)


def test_the_scenes_of_the_device_tests():
    gt, pred = mm.composed_scene()
    assert gt.shape == (41, 45) and mm.margin(gt) >= 2 and mm.margin(pred) >= 2
    m = gt > 0
    import clean_ref
    assert clean_ref.label(m, 4)[1] == clean_ref.label(m, 8)[1] + 1                     # the diagonal pair: one contact, corners only
    assert clean_ref.clean(m.astype(np.uint8))["info"][0] == 1                         # one hole
    assert (gt == 7).sum() == 1 and (measure_ref.edge_counts(gt)[2][gt == 1] > 0).any() # a one-pixel cell; cells 1 and 2 touch
    bridge = (gt == 4) & (np.roll(gt, 1, 0) != 4) & (np.roll(gt, -1, 0) != 4)
    assert bridge.sum() >= 3                                                           # the one-pixel bridge
    g, p = mm.strip_scene()
    assert g.shape == (3, 40) and not any(m[:, c].any() for m in (g, p) for c in (0, -1)) and (p > 0).sum() > 60


# ---- the placement plan -----------------------------------------------------------------------------------------------------

def test_placement_plan_meets_the_seam_conditions():
    plan = mm.placements(41, 45)
    assert len(plan) <= 48 and len(set(plan)) == len(plan) and (0, 0) in plan
    assert mm.seam_gaps(plan, 41, 45) == []
    H, W = mm.CANVAS
    assert all(0 <= dy <= H - 41 and 0 <= dx <= W - 45 for dy, dx in plan)
    assert {dy for dy, _ in plan} >= set(mm.OFFSETS_Y) and {dx for _, dx in plan} >= set(mm.OFFSETS_X)
    # a plan without the placements next to a seam, or without the last row, is found wanting
    assert mm.seam_gaps([p for p in plan if p[0] != 63], 41, 45) == ["axis 0: no start at 63"]
    assert mm.seam_gaps([p for p in plan if p[1] != W - 45], 41, 45) == ["axis 1: no placement ends at the canvas's end"]
    assert "axis 1: no seam of period 64 inside the scene" in mm.seam_gaps([(0, 0), (0, 64)], 3, 5)
    even = mm.placements(41, 45, lattice=2)
    assert len(even) <= 48 and all(dy % 2 == 0 and dx % 2 == 0 for dy, dx in even) and mm.seam_gaps(even, 41, 45, lattice=2) == []
    strip = mm.placements(3, 40, mm.STRIP_CANVAS, (0,), mm.STRIP_X)
    assert sorted(dx for _, dx in strip) == sorted(mm.STRIP_X) and all(dy == 0 for dy, _ in strip)
    assert any(dx < 256 < dx + 39 for _, dx in strip) and {255, 256} <= {dx for _, dx in strip}     # the 256-pixel row chunk ends inside
    assert max(dx for _, dx in strip) + 40 == mm.STRIP_CANVAS[1]


# ---- deliberately broken ops are caught -----------------------------------------------------------------------------------

def nearest_with_rule(key):
    """grow_cells by brute force with another rule among the labelled pixels at the least distance: the one with the least key(id,
    y, x) gives its id."""
    def grow(x, max_distance=None):
        out = []
        for lab in x["ids"].astype(np.int64):
            ys, xs = np.nonzero(lab)
            res = lab.copy()
            for y, xx in zip(*np.nonzero(lab == 0)):
                d = (ys - y) ** 2 + (xs - xx) ** 2
                near = np.flatnonzero(d == d.min())
                res[y, xx] = min((key(lab[ys[k], xs[k]], ys[k], xs[k]), lab[ys[k], xs[k]]) for k in near)[1]
            out.append(res)
        return {"out": np.stack(out)}
    return grow


def tie_scene(a, b):
    """Two cells a and b, mirror images about a background column whose pixels are equally far from both."""
    lab = np.zeros((1, 5, 9), np.int32)
    lab[0, 1:4, 1:3], lab[0, 1:4, 6:8] = b, a
    return {"ids": lab}


def test_a_tie_that_goes_to_the_first_pixel_in_raster_order_is_caught_by_D():
    """The labeller broken here is the nearest-cell one (grow_cells): label_cells has no tie to give away, its numbering by the
    first pixel in raster order is its definition and canon_labels takes it out."""
    raster = nearest_with_rule(lambda i, y, x: (y, x))
    x = tie_scene(1, 2)
    mm.relation_D("grow_cells", tie_scene(2, 1), "ref")                                  # the stated rule passes on both
    mm.relation_D("grow_cells", x, "ref")
    with pytest.raises(AssertionError, match="view"):
        mm.relation_D("grow_cells", x, raster)


def test_a_nearest_id_rule_that_ignores_id_order_is_caught_by_R():
    rule = nearest_with_rule(lambda i, y, x: i % 4)                                      # cells 1 and 4: 4 wins; 3 i + 5 gives 8 and 17: 8 wins
    x = tie_scene(1, 4)
    mm.relation_R("grow_cells", x, "ref", mm.order_map)
    mm.relation_D("grow_cells", x, rule)                                                 # D does not see it: the rule is geometric
    with pytest.raises(AssertionError, match="renamed"):
        mm.relation_R("grow_cells", x, rule, mm.order_map)


def test_a_distance_map_that_drops_column_64_of_each_65_wide_block_is_caught_by_T():
    def broken(x):
        out = []
        for m in x["mask"]:
            seen = m.copy()
            seen[:, 64::65] = 1                                                          # background there is never looked at
            out.append(shape_ref.distance2(seen, "ignore") * (m != 0))
        return {"d2": np.stack(out)}
    scene = np.zeros((1, 8, 9), np.uint8)
    scene[0, 2:6, 2:7] = 1
    scene[0, 3, 4] = 0                                                                   # a hole: the nearest background of the pixels round it
    x = {"mask": scene}
    plan = [(0, 0), (1, 58), (2, 60), (0, 71)]                                           # at dx = 60 the hole lies in column 64
    assert mm.relation_T("distance_map[ignore]", x, "ref", (12, 80), plan) == 3
    with pytest.raises(AssertionError, match=r"scene at \(2, 60\)"):
        mm.relation_T("distance_map[ignore]", x, broken, (12, 80), plan)
    mm.relation_D("distance_map[ignore]", x, broken)                                     # an 8 x 9 image has no column 64: D passes


def test_a_sum_that_leaks_a_pixel_into_the_next_image_is_caught_by_B(scene):
    def broken(x):
        r = measure_ref.sums_batch(x["ids"], x["image16"])
        for b in range(1, len(x["ids"])):
            i = x["ids"][b - 1][-1, -1]
            r["area"][b, i] += 1
            r["present"][b, i] = True
        return r
    mm.relation_D("cell_sums", scene, broken)                                            # one image: nothing leaks
    with pytest.raises(AssertionError, match="batch"):
        mm.relation_B("cell_sums", scene, broken)
