"""Per-cell convex hulls and neighbours on the device (functions.cell_hulls / hull_props / cell_neighbours -> unet_cell_hulls,
unet_cell_contacts) against the Python-integer restatement tests/hull_ref.py (pinned to hand-worked answers and to
scipy.spatial.ConvexHull by tests/test_hull_cpu.py).  Every output and status word is compared bit for bit, vertices in the stated
order and the zero tails of the slices included, and every case runs twice.  Every pointer handed to the raw entry points is a
poisoned guarded.Arena buffer."""
import functools

import numpy as np
import pytest
import torch

import guarded
import hull_ref as ref
import measure_ref
from gpu_support import dev, hip, rejected  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CODE = {torch.int64: 0, torch.int32: 2}
FIELDS = ("n_vertices", "area2", "feret_max2", "width", "vertices")


def boxes_and_offsets(labels, n_max):
    """What the caller of unet_cell_hulls forms: unet_cell_sums's boxes [B, N, 4] and the prefix sum of the level counts."""
    s = measure_ref.sums_batch(labels, None, n_max)
    levels = np.where(s["present"], s["bbox"][..., 2] - s["bbox"][..., 0] + 1, 0).astype(np.int64)
    levels[:, 0] = 0
    return s["bbox"], np.concatenate([[0], np.cumsum(levels.ravel())]).astype(np.int64)


def raw_hulls(dev, labels, n_max, ldtype=torch.int32, bbox=None, offset=None, n_levels=None, expect_status=(0, 0), null_tables=False):
    """unet_cell_hulls on guarded buffers: a dict like hull_ref.hulls's (without the offsets); labels numpy [B,H,W]."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = labels.shape
    N = n_max + 1
    if bbox is None:
        bbox, offset = boxes_and_offsets(labels, n_max)
    nl = int(offset[-1]) if n_levels is None else n_levels
    lab = a.inp(torch.from_numpy(labels).to(ldtype), "labels")
    box, off = a.inp(torch.from_numpy(np.ascontiguousarray(bbox, np.int32)), "bbox"), a.inp(torch.from_numpy(np.ascontiguousarray(offset, np.int64)), "offset")
    nv, a2, f2 = a.out((B, N), torch.int32, "n_vertices"), a.out((B, N), torch.int64, "area2"), a.out((B, N), torch.int64, "feret_max2")
    wd, vt, status = a.out((B, N, 2), torch.int64, "width"), a.out((2 * nl, 2), torch.int32, "vertices"), a.out((B, 2), torch.int64, "status")
    scratch = a.scratch(L.unet_cell_hulls_scratch_bytes(nl), "scratch")
    _hip.run("unet_cell_hulls", dev, a.ptr(lab), CODE[ldtype], B, H, W, n_max, a.ptr(box), a.ptr(off), nl, a.ptr(nv), a.ptr(a2), a.ptr(f2), a.ptr(wd),
             None if null_tables else a.ptr(vt), a.ptr(status), None if null_tables else a.ptr(scratch))
    a.verify(nv, a2, f2, wd, vt, status)
    assert torch.equal(lab.cpu(), torch.from_numpy(labels).to(ldtype)) and torch.equal(off.cpu(), torch.from_numpy(np.asarray(offset, np.int64)))
    assert status.cpu().sum(dim=0).tolist() == list(expect_status)
    return {"n_vertices": nv.cpu().numpy(), "area2": a2.cpu().numpy(), "feret_max2": f2.cpu().numpy(), "width": wd.cpu().numpy(),
            "vertices": vt.cpu().numpy()}


def wrapped(dev, labels, n_max, ldtype, with_sums):
    import functions
    lab = torch.from_numpy(labels).to(dev).to(ldtype)
    h = functions.cell_hulls(lab, functions.cell_sums(lab, n_max=n_max), n_max=n_max) if with_sums else functions.cell_hulls(lab, n_max=n_max)
    assert isinstance(h, functions.CellHulls) and all(t.is_cuda for t in h)
    return {"n_vertices": h.n_vertices.cpu().numpy(), "area2": h.area2.cpu().numpy(), "feret_max2": h.feret_max2.cpu().numpy(),
            "width": torch.stack([h.width_cross, h.width_len2], dim=-1).cpu().numpy(), "vertices": h.vertices.cpu().numpy(),
            "offset": h.offset.cpu().numpy()}


def same(got, want, what):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def raw_contacts(dev, labels, n_max, ldtype=torch.int32, slots=None, expect_bad=0, may_drop=False):
    """unet_cell_contacts on guarded buffers -> ((b, i, j, sides) sorted, dropped sides)."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = labels.shape
    slots = 1 << int(2 * labels.size + 8).bit_length() if slots is None else slots
    lab = a.inp(torch.from_numpy(labels).to(ldtype), "labels")
    keys, counts = a.out((slots,), torch.int64, "pair_keys"), a.out((slots,), torch.int32, "pair_counts")
    n_pairs, status = a.out((1,), torch.int64, "n_pairs"), a.out((B, 2), torch.int64, "status")
    scratch = a.scratch(L.unet_cell_contacts_scratch_bytes(B, slots), "scratch")
    _hip.run("unet_cell_contacts", dev, a.ptr(lab), CODE[ldtype], B, H, W, n_max, slots, a.ptr(keys), a.ptr(counts), a.ptr(n_pairs), a.ptr(status),
             a.ptr(scratch))
    a.verify(n_pairs, status)
    bad, dropped = status.cpu().sum(dim=0).tolist()
    assert bad == expect_bad and (may_drop or dropped == 0) and torch.equal(lab.cpu(), torch.from_numpy(labels).to(ldtype))
    n = int(n_pairs.item())
    assert 0 <= n <= slots
    k, c = keys.cpu().numpy().view(np.uint64), counts.cpu().numpy()
    assert (k[n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (c[n:] == -1).all()          # the rest of the lists is untouched
    order = np.argsort(k[:n])
    k, c = k[:n][order], c[:n][order].astype(np.int64)
    assert len(np.unique(k)) == n
    return tuple((k >> np.uint64(s) & np.uint64(m)).astype(np.int64) for s, m in ((48, 0xFFFF), (24, 0xFFFFFF), (0, 0xFFFFFF))) + (c,), dropped


def same_contacts(got, want, what):
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), what


@functools.lru_cache(maxsize=None)
def maps(H, W):
    """The named id maps of one size with their n_max (larger than the largest id) and their reference: (name, [B,H,W], n_max, hulls,
    contacts).  The references are computed once and shared."""
    out = [("blocks", np.stack([ref.block_map(s * 100 + H + W, H, W) for s in (1, 2, 3)]), None),
           ("one id", np.full((1, H, W), 7, np.int32), 9),
           ("own ids", measure_ref.every_pixel_its_own(H, W)[None], H * W + 1),
           ("sparse, in parts", np.stack([ref.sparse_ids(H, W), np.zeros((H, W), np.int32), ref.sparse_ids(H, W)[::-1, ::-1]]), 70003),
           ("empty", np.zeros((3, H, W), np.int32), 4)]
    pair = ref.disc_pair()
    for p in (pair, pair.T):
        if H >= p.shape[0] and W >= p.shape[1]:
            m = np.zeros((2, H, W), np.int32)
            m[0, H - p.shape[0]:, W - p.shape[1]:] = p * 5
            m[1, :25, :25][ref.disc()] = 2
            out.append(("discs", m, 6))
            break
    done = []
    for name, m, n_max in out:
        m = np.ascontiguousarray(m, np.int32)
        n_max = int(m.max()) + 3 if n_max is None else n_max
        done.append((name, m, n_max, ref.hulls(m, n_max), ref.contacts(m, n_max)))
    return done


def check_hulls(dev, m, n_max, want, what, ldtypes=(torch.int32, torch.int64)):
    for ldtype in ldtypes:
        one, two = raw_hulls(dev, m, n_max, ldtype), raw_hulls(dev, m, n_max, ldtype)
        same(one, want, (what, ldtype, "raw"))
        same(two, one, (what, ldtype, "two runs"))
        got = wrapped(dev, m, n_max, ldtype, with_sums=ldtype == torch.int32)
        same(got, want, (what, ldtype, "wrapper"))
        assert np.array_equal(got["offset"], want["offset"])


# ---- sizes, batches, label dtypes -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", ref.SIZES)
def test_sizes(dev, H, W):
    """Every map of the size, B 1-3, int32 and int64 labels, n_max above the largest id: hulls and contacts bit for bit, twice, raw
    and wrapped."""
    names = set()
    for name, m, n_max, want, pairs in maps(H, W):
        check_hulls(dev, m, n_max, want, (name, H, W))
        for ldtype in (torch.int32, torch.int64):
            one, two = raw_contacts(dev, m, n_max, ldtype)[0], raw_contacts(dev, m, n_max, ldtype)[0]
            same_contacts(one, pairs, (name, H, W, ldtype))
            same_contacts(two, one, (name, H, W, ldtype, "two runs"))
        if name == "one id":
            assert want["n_vertices"][0, 7] == 4 and want["area2"][0, 7] == 2 * H * W and want["vertices"].shape == (2 * (H + 1), 2)
        if name == "own ids":
            assert (want["n_vertices"][0, 1:H * W + 1] == 4).all() and (want["area2"][0, 1:H * W + 1] == 2).all()
            assert len(pairs[0]) == H * (W - 1) + (H - 1) * W and (pairs[3] == 1).all()
        if name == "empty":
            assert want["vertices"].shape == (0, 2) and not want["n_vertices"].any()
            same(raw_hulls(dev, m, n_max, null_tables=True), want, "L = 0 with NULL vertices and scratch")
        if name == "discs":
            assert want["area2"][0, 5] == 2046 and want["area2"][1, 2] == 946 and want["n_vertices"][1, 2] == 24
        names.add(name)
    assert names >= {"blocks", "one id", "own ids", "sparse, in parts", "empty"} and ("discs" in names) == (min(H, W) >= 27 and max(H, W) >= 49)


def test_strip_needs_128_bits(dev):
    """The input of test_hull_cpu.test_strip_needs_more_than_64_bits: a comparison in wrapped 64-bit products picks another edge."""
    m = ref.strip_case()[None]
    want = ref.hulls(m, 2)
    v = [tuple(p) for p in want["vertices"][:want["n_vertices"][0, 1]].tolist()]
    assert tuple(want["width"][0, 1].tolist()) == ref.measure(v)[2] != ref.measure(v, ref.less_wrapped64)[2]
    check_hulls(dev, m, 2, want, "strip")
    both = np.concatenate([m, m[:, ::-1, ::-1]])
    check_hulls(dev, both, 1, ref.hulls(both, 1), "strip, both ways", ldtypes=(torch.int32,))


# ---- what the entries refuse ------------------------------------------------------------------------------------------------

def test_ids_out_of_range(dev):
    """Status word 0 counts them, and the hulls and contacts of the other ids are exact."""
    m = np.stack([ref.block_map(5, 37, 300), ref.block_map(6, 37, 300)])
    n_max = int(m.max())
    bad = m.copy()
    bad[0, 3, 60:70], bad[1, 36, 290:], bad[1, 0, 0], bad[0, 20, 5] = n_max + 1, -1, 1 << 24, -(1 << 30)
    clean = np.where((bad < 0) | (bad > n_max), 0, bad)
    bbox, offset = boxes_and_offsets(clean, n_max)
    want = ref.hulls(clean, n_max)
    for ldtype in (torch.int32, torch.int64):
        same(raw_hulls(dev, bad, n_max, ldtype, bbox, offset, expect_status=(22, 0)), want, ldtype)
    # a refused pixel is nobody's neighbour: the reference drops the pairs that hold one
    same_contacts(raw_contacts(dev, bad, n_max, expect_bad=22)[0], ref.contacts(np.where((bad < 0) | (bad > n_max), -5, bad), n_max), "contacts")
    import functions
    lab = torch.from_numpy(bad).to(dev)
    with pytest.raises(ValueError, match="negative"):
        functions.cell_hulls(lab)
    with pytest.raises(ValueError, match="negative"):
        functions.cell_neighbours(lab)
    with pytest.raises(ValueError, match="outside"):
        functions.cell_hulls(lab.clamp(min=0), n_max=n_max)
    sums = functions.cell_sums(torch.from_numpy(clean).to(dev), n_max=n_max)
    with pytest.raises(ValueError, match="outside"):
        functions.cell_hulls(lab, sums)
    with pytest.raises(ValueError, match="sums"):
        functions.cell_hulls(lab[0], sums)


def test_shrunken_box_and_wrong_offsets(dev):
    """Status word 1 counts the pixels outside the box given for their id, and those of an id whose level count does not fit; no
    byte outside the buffers or inside the guards is touched (raw_hulls verifies the guards), the other rows are exact."""
    m = np.stack([ref.block_map(8, 37, 300), ref.block_map(9, 37, 300)])
    n_max = int(m.max()) + 2
    N = n_max + 1
    bbox, offset = boxes_and_offsets(m, n_max)
    h, w = bbox[..., 2] - bbox[..., 0], bbox[..., 3] - bbox[..., 1]
    b, i = [int(v[0]) for v in np.nonzero((h >= 4) & (w >= 4) & (np.arange(N) > 0))]
    small = bbox.copy()
    small[b, i] += np.array([1, 1, -1, -1], np.int32)
    levels = np.diff(offset)
    levels[b * N + i] -= 2
    off2 = np.concatenate([[0], np.cumsum(levels)])
    y0, x0, y1, x1 = small[b, i]
    inside = np.zeros(m.shape, bool)
    inside[b, y0:y1, x0:x1] = True
    lost = int(((m == i) & (np.arange(len(m))[:, None, None] == b) & ~inside).sum())
    assert lost > 0
    want = ref.hulls(m, n_max, bbox=small)
    assert np.array_equal(want["offset"], off2)
    for ldtype in (torch.int32, torch.int64):
        same(raw_hulls(dev, m, n_max, ldtype, small, off2, expect_status=(0, lost)), want, "shrunken box")
    # a box that no longer matches its level count: the row gives nothing, all its pixels are counted
    area = int(((m == i) & (np.arange(len(m))[:, None, None] == b)).sum())
    gone = m.copy()
    gone[b][m[b] == i] = 0
    want = ref.hulls(gone, n_max)                                                             # every other row is as without that id
    one_less = np.concatenate([offset[:b * N + i + 1], offset[b * N + i + 1:] - 1])          # row (b, i) is one level short
    got = raw_hulls(dev, m, n_max, torch.int32, bbox, one_less, expect_status=(0, area))
    for k in FIELDS[:-1]:
        assert np.array_equal(got[k], want[k]), k
    # its vertices: every other row's slice where the shifted table puts it, the rest 0
    expect = np.zeros((2 * int(one_less[-1]), 2), np.int32)
    for r in range(len(m) * N):
        k = int(want["n_vertices"].ravel()[r])
        expect[2 * one_less[r]:2 * one_less[r] + k] = want["vertices"][2 * want["offset"][r]:2 * want["offset"][r] + k]
    assert np.array_equal(got["vertices"], expect)
    # offsets that are no prefix sum at all: nothing is written but zeros, every foreground pixel is counted
    rs = np.random.RandomState(0)
    wild = rs.randint(-(1 << 62), 1 << 62, offset.shape).astype(np.int64)
    wild[::3] = rs.randint(-5, int(offset[-1]) + 5, wild[::3].shape)
    for table in (wild, offset[::-1].copy(), offset * 2, np.full_like(offset, -1)):
        got = raw_hulls(dev, m, n_max, torch.int64, bbox, table, n_levels=int(offset[-1]), expect_status=(0, int((m > 0).sum())))
        assert not any(got[k].any() for k in FIELDS)
    wide = bbox.copy()                                                                          # boxes outside the image
    wide[..., 2] += 40
    wide[..., 3] = 301
    got = raw_hulls(dev, m, n_max, torch.int32, wide, offset, expect_status=(0, int((m > 0).sum())))
    assert not any(got[k].any() for k in FIELDS)


def test_a_rejected_call_writes_nothing(dev, hip):
    L = hip.lib()
    a = guarded.Arena(dev)
    B, H, W, n_max = 2, 9, 11, 4
    N = n_max + 1
    m = np.ones((B, H, W), np.int32)
    bbox, offset = boxes_and_offsets(m, n_max)
    nl = int(offset[-1])
    lab, box, off = a.inp(torch.from_numpy(m), "labels"), a.inp(torch.from_numpy(bbox), "bbox"), a.inp(torch.from_numpy(offset), "offset")
    nv, a2, f2 = a.out((B, N), torch.int32, "n_vertices"), a.out((B, N), torch.int64, "area2"), a.out((B, N), torch.int64, "feret_max2")
    wd, vt, status = a.out((B, N, 2), torch.int64, "width"), a.out((2 * nl, 2), torch.int32, "vertices"), a.out((B, 2), torch.int64, "status")
    scratch = a.scratch(L.unet_cell_hulls_scratch_bytes(nl), "scratch")
    st = hip.stream(dev)
    p = a.ptr
    good = dict(lab=p(lab), ld=2, B=B, H=H, W=W, n=n_max, box=p(box), off=p(off), L=nl, nv=p(nv), a2=p(a2), f2=p(f2), wd=p(wd), vt=p(vt),
                status=p(status), scratch=p(scratch))
    for bad in ({"ld": 1}, {"ld": 3}, {"ld": -1}, {"lab": None}, {"box": None}, {"off": None}, {"nv": None}, {"a2": None}, {"f2": None},
                {"wd": None}, {"vt": None}, {"scratch": None}, {"status": None}, {"B": 0}, {"H": 0}, {"W": -1}, {"H": 32769, "W": 1},
                {"H": 1, "W": 32769}, {"B": 70000}, {"n": -1}, {"n": 1 << 24}, {"L": -1}):
        kw = dict(good, **bad)
        rc = L.unet_cell_hulls(kw["lab"], kw["ld"], kw["B"], kw["H"], kw["W"], kw["n"], kw["box"], kw["off"], kw["L"], kw["nv"], kw["a2"], kw["f2"],
                               kw["wd"], kw["vt"], kw["status"], kw["scratch"], st)
        rejected(hip, rc, a, nv, a2, f2, wd, vt, status, scratch)
        assert b"unet_cell_hulls" in L.unet_last_error()
    slots = 64
    keys, counts, n_pairs = a.out((slots,), torch.int64, "pair_keys"), a.out((slots,), torch.int32, "pair_counts"), a.out((1,), torch.int64, "n_pairs")
    table = a.scratch(L.unet_cell_contacts_scratch_bytes(B, slots), "table")
    good = dict(lab=p(lab), ld=2, B=B, H=H, W=W, n=n_max, slots=slots, keys=p(keys), counts=p(counts), np=p(n_pairs), status=p(status), scratch=p(table))
    for bad in ({"ld": 1}, {"ld": 4}, {"lab": None}, {"keys": None}, {"counts": None}, {"np": None}, {"status": None}, {"scratch": None}, {"B": 0},
                {"W": 0}, {"H": 40000}, {"W": 32769}, {"B": 65536}, {"n": -1}, {"n": 1 << 24}, {"slots": 0}, {"slots": 48}):
        kw = dict(good, **bad)
        rc = L.unet_cell_contacts(kw["lab"], kw["ld"], kw["B"], kw["H"], kw["W"], kw["n"], kw["slots"], kw["keys"], kw["counts"], kw["np"],
                                  kw["status"], kw["scratch"], st)
        rejected(hip, rc, a, keys, counts, n_pairs, status, table)
        assert b"unet_cell_contacts" in L.unet_last_error()


# ---- contacts: a full table, the sum invariant ------------------------------------------------------------------------------

def test_a_full_table_reports_and_cell_neighbours_recovers(dev):
    import functions
    m = np.stack([measure_ref.every_pixel_its_own(9, 13), ref.block_map(4, 9, 13)])
    want = ref.contacts(m)
    assert len(want[0]) > 200
    got, dropped = raw_contacts(dev, m, int(m.max()), slots=32, may_drop=True)
    assert dropped > 0 and len(got[0]) <= 32 and dropped + int(got[3].sum()) == int(want[3].sum())
    held = {(b, i, j): n for b, i, j, n in zip(*(x.tolist() for x in want))}
    assert all(held.get((b, i, j), 0) >= n > 0 for b, i, j, n in zip(*(x.tolist() for x in got)))
    for ldtype in (torch.int32, torch.int64):
        nb = functions.cell_neighbours(torch.from_numpy(m).to(dev).to(ldtype), _table_slots=32)
        assert isinstance(nb, functions.Neighbours)
        same_contacts(nb, want, "doubling")
    same_contacts(functions.cell_neighbours(torch.from_numpy(m[1]).to(dev)), ref.contacts(m[1]), "one image, the default table")


def test_contacts_sum_to_cell_sums_contact_on_the_device(dev):
    import functions
    m = np.stack([ref.block_map(11, 129, 97), ref.block_map(12, 129, 97), ref.sparse_ids(129, 97, 300)])
    lab = torch.from_numpy(m).to(dev)
    nb, sums = functions.cell_neighbours(lab), functions.cell_sums(lab)
    n_max = int(m.max())
    total = np.zeros((3, n_max + 1), np.int64)
    np.add.at(total, (nb.b, nb.i), nb.sides)
    np.add.at(total, (nb.b, nb.j), nb.sides)
    assert np.array_equal(total[:, 1:], sums.contact.cpu().numpy()[:, 1:]) and total.sum() > 1000
    counts = functions.neighbour_counts(nb, 3, n_max)
    assert np.array_equal(counts > 0, total > 0) and counts.max() >= 3


# ---- the wrapper ------------------------------------------------------------------------------------------------------------

def test_cell_hulls_with_and_without_sums_and_hull_props(dev):
    import functions
    m = np.zeros((2, 64, 100), np.int32)
    p = ref.disc_pair()
    m[0, 3:3 + p.shape[0], 5:5 + p.shape[1]] = p * 3
    m[0, 35:60, 60:85][ref.disc()] = 1
    m[1] = ref.block_map(13, 64, 100)
    lab = torch.from_numpy(m).to(dev)
    sums = functions.cell_sums(lab)
    a, b = functions.cell_hulls(lab), functions.cell_hulls(lab, sums)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = functions.cell_hulls(lab.long(), sums)
    side.synchronize()
    for f in functions.CellHulls._fields:
        assert torch.equal(getattr(a, f), getattr(b, f)) and torch.equal(getattr(a, f), getattr(c, f)), f
    want = ref.hulls(m, int(m.max()))
    props = functions.hull_props(a, sums)
    assert props.solidity.shape == (2, int(m.max()) + 1)
    assert round(float(props.solidity[0, 3]), 3) == 0.851 and round(float(props.solidity[0, 1]), 3) == 0.932
    on = want["n_vertices"] > 0
    assert np.array_equal(np.isfinite(props.solidity), on) and (props.solidity[on] <= 1).all()
    assert np.array_equal(props.convex_area[on], want["area2"][on] / 2) and np.array_equal(props.feret_max[on], np.sqrt(want["feret_max2"][on]))
    single = functions.cell_hulls(lab[0])
    assert single.n_vertices.shape == (4,) and single.offset.shape == (5,)
    k = int(single.n_vertices[3])
    assert np.array_equal(single.vertices.cpu().numpy()[2 * int(single.offset[3]):][:k], want["vertices"][2 * int(want["offset"][3]):][:k])
    ps = functions.hull_props(single, functions.cell_sums(lab[0]))
    assert np.array_equal(ps.solidity, props.solidity[0, :4], equal_nan=True) and np.array_equal(ps.convex_perimeter, props.convex_perimeter[0, :4], equal_nan=True)
    with pytest.raises(NotImplementedError):
        functions.cell_hulls(lab.cpu())
    with pytest.raises(NotImplementedError):
        functions.cell_hulls(lab, functions.CellSums(*(None if t is None else t.cpu() for t in sums)))
    with pytest.raises(ValueError, match="n_max"):
        functions.cell_hulls(lab, sums, n_max=int(m.max()) + 1)
