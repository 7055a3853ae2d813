"""The numpy restatement of the shape ops (tests/shape_ref.py), which tests/test_shape_gpu.py holds the device ops to, pinned on
the CPU: the distance map against scipy's exact transform, the reconstruction against a priority-queue algorithm, the seed count
against a count of the maxima by their dynamics (union-find over the pixels in descending height), the regional maxima against a
plateau search, and all of it against hand-worked answers; and that the inputs of the GPU tests exercise the code.  And the new
entry points: declared, in the ctypes table and in the library."""
import functools
import heapq
import os
import re

import numpy as np
import pytest
from scipy import ndimage, sparse
from scipy.sparse import csgraph

import shape_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_distance_map_scratch_bytes", "unet_distance_map", "unet_reconstruct_scratch_bytes", "unet_reconstruct_init",
       "unet_reconstruct_sweeps", "unet_reconstruct_finish", "unet_shape_heights", "unet_shape_lower", "unet_shape_maxima")


def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert L.unet_distance_map_scratch_bytes(2, 33, 31) >= 2 * 33 * 31 * 4
    assert L.unet_reconstruct_scratch_bytes(2, 33, 31) >= 2 * 33 * 31 * 16    # two planes of R, under, min(marker, under)
    assert L.unet_distance_map_scratch_bytes(2, 0, 31) == 0 and L.unet_reconstruct_scratch_bytes(0, 3, 3) == 0


def test_library_refuses_bad_arguments_before_any_launch():
    """ARG_CHECK answers on the host: no device is needed to be refused."""
    import ctypes as C
    import _hip
    _hip.build()
    L = _hip.lib()
    q = C.c_void_p(4096)                                     # never dereferenced: every call below is refused first
    assert L.unet_distance_map(q, 4, 1, 8, 8, 0, q, q, None) == -2 and b"dtype" in L.unet_last_error()
    assert L.unet_distance_map(q, 0, 1, 8, 8, 2, q, q, None) == -2 and b"edge" in L.unet_last_error()
    assert L.unet_distance_map(None, 0, 1, 8, 8, 0, q, q, None) == -2
    assert L.unet_distance_map(q, 0, 1, 8, 8, 0, None, q, None) == -2
    assert L.unet_distance_map(q, 0, 1, 8, 8, 0, q, None, None) == -2
    assert L.unet_distance_map(q, 0, 1, 32768, 1, 0, q, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_distance_map(q, 0, 1, 1, 32768, 0, q, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_distance_map(q, 0, 70000, 8, 8, 0, q, q, None) == -2
    assert L.unet_reconstruct_init(q, 1, q, 0, None, 0, 1, 8, 8, q, q, None) == -2 and b"dtype" in L.unet_last_error()
    assert L.unet_reconstruct_init(q, 0, q, 3, None, 0, 1, 8, 8, q, q, None) == -2
    assert L.unet_reconstruct_init(q, 0, q, 0, q, 4, 1, 8, 8, q, q, None) == -2
    assert L.unet_reconstruct_init(None, 0, q, 0, None, 0, 1, 8, 8, q, q, None) == -2
    assert L.unet_reconstruct_init(q, 0, None, 0, None, 0, 1, 8, 8, q, q, None) == -2
    assert L.unet_reconstruct_init(q, 0, q, 0, None, 0, 1, 8, 8, None, q, None) == -2
    assert L.unet_reconstruct_init(q, 0, q, 0, None, 0, 1, 8, 8, q, None, None) == -2
    assert L.unet_reconstruct_init(q, 0, q, 0, None, 0, 1, 40000, 8, q, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_reconstruct_sweeps(1, 8, 8, 0, q, 0, q, None) == -2
    assert L.unet_reconstruct_sweeps(1, 8, 8, 1, None, 0, q, None) == -2
    assert L.unet_reconstruct_sweeps(1, 8, 8, 1, q, -1, q, None) == -2
    assert L.unet_reconstruct_sweeps(1, 8, 8, 1, q, 0, None, None) == -2
    assert L.unet_reconstruct_finish(1, 8, 8, None, q, q, None) == -2
    assert L.unet_reconstruct_finish(1, 8, 8, q, None, q, None) == -2
    assert L.unet_reconstruct_finish(1, 8, 8, q, q, None, None) == -2
    assert L.unet_shape_heights(q, 1, 8, 8, -1, q, q, None) == -2 and b"hq" in L.unet_last_error()
    assert L.unet_shape_heights(q, 1, 8, 8, (1 << 28) + 1, q, q, None) == -2
    assert L.unet_shape_heights(None, 1, 8, 8, 0, q, q, None) == -2
    assert L.unet_shape_heights(q, 1, 8, 8, 0, None, q, None) == -2
    assert L.unet_shape_lower(q, 1, 8, 8, -1, q, None) == -2
    assert L.unet_shape_lower(q, 1, 8, 8, 1, None, None) == -2
    assert L.unet_shape_maxima(q, None, 1, 8, 8, 0, q, None) == -2
    assert L.unet_shape_maxima(q, q, 1, 8, 8, 0, None, None) == -2


# ---- the inputs of the GPU tests, and what is computed once for them -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_masks():
    """[(name, mask [H,W])]: every image of every size case."""
    return [("%dx%d %s [%d]" % (H, W, name, b), m[b]) for H, W in ref.SIZES for name, m in ref.size_cases(H, W) for b in range(len(m))]


@functools.lru_cache(maxsize=None)
def maxima_of(k, h, edge):
    """(q, R1, R2) of image k of all_masks()."""
    region = all_masks()[k][1] != 0
    q = ref.heights(region, edge)
    return (q,) + ref.h_maxima(q, region, ref.quanta(h, 0)[0])


def edt2(region, edge):
    if edge == "background":
        return edt2(np.pad(region, 1), "ignore")[1:-1, 1:-1]
    if region.all():
        return np.full(region.shape, region.shape[0] ** 2 + region.shape[1] ** 2, np.int64)
    return np.rint(ndimage.distance_transform_edt(region) ** 2).astype(np.int64)


def count_by_dynamics(q, region, hq):
    """The maxima of q on the region whose dynamic exceeds hq: flood the region in descending q; when two flooded parts meet at
    height v, the one with the lower peak ends there, with the dynamic peak - v; the highest peak of each region component never
    ends and counts as infinite."""
    H, W = q.shape
    flat = np.flatnonzero(region.ravel())
    order = flat[np.argsort(-q.ravel()[flat], kind="stable")]
    parent, peak = {}, {}

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    qf = q.ravel()
    count = 0
    for i in order.tolist():
        v = int(qf[i])
        parent[i], peak[i] = i, v
        y, x = divmod(i, W)
        for j in ((i - W) if y > 0 else -1, (i + W) if y < H - 1 else -1, (i - 1) if x > 0 else -1, (i + 1) if x < W - 1 else -1):
            if j < 0 or j not in parent:
                continue
            a, b = find(i), find(j)
            if a == b:
                continue
            lo, hi = (a, b) if peak[a] <= peak[b] else (b, a)
            count += peak[lo] - v > hq
            parent[lo] = hi
    return count + sum(1 for i in parent if parent[i] == i)


def plateau_maxima(R, region):
    """bool [H,W]: the region pixels of the 4-connected plateaus of R that have no higher region neighbour."""
    H, W = R.shape
    idx = np.arange(H * W).reshape(H, W)
    rows, cols = [], []
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        same = region[a] & region[b] & (R[a] == R[b])
        rows.append(idx[a][same])
        cols.append(idx[b][same])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    graph = sparse.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(H * W, H * W))
    _, lab = csgraph.connected_components(graph, directed=False)
    lab = lab.reshape(H, W)
    higher = ref.neighbour_max(np.where(region, R, ref.LOW)) > R
    dominated = np.bincount(lab[region & higher], minlength=lab.max() + 1) > 0
    return region & ~dominated[lab]


# ---- pins -------------------------------------------------------------------------------------------------------------------

def test_distance_map_equals_scipy():
    for name, m in all_masks():
        region = m != 0
        for edge in ref.EDGES:
            d2 = ref.distance2(region, edge)
            assert np.array_equal(d2, edt2(region, edge)), (name, edge)
            assert (d2[~region] == 0).all()
            if region.size <= 66 * 66:
                assert np.array_equal(d2, ref.distance2_brute(region, edge)), (name, edge, "brute")
    yy, xx = np.mgrid[0:9, 0:7]
    full = np.ones((9, 7), bool)
    assert (ref.distance2(full) == 81 + 49).all()
    assert np.array_equal(ref.distance2(full, "background"), np.minimum(np.minimum(xx + 1, 7 - xx), np.minimum(yy + 1, 9 - yy)) ** 2)


def test_isqrt256():
    v = np.concatenate([np.arange(0, 5000), (np.arange(1, 46341, dtype=np.int64) ** 2)[-2000:], [2 ** 31 - 1, 32767 ** 2 * 2]])
    q = ref.isqrt256(v)
    assert (q * q <= 256 * v).all() and ((q + 1) ** 2 > 256 * v).all()
    assert ref.isqrt256(np.array([0, 1, 2, 144, 49]))[[0, 1, 3, 4]].tolist() == [0, 16, 192, 112] and ref.isqrt256(np.array([2]))[0] == 22


def widest_paths(marker, under, region):
    """The reconstruction by a priority queue: pixels leave the queue in descending value, each offers min(under(n), its value)."""
    R = np.where(region, np.minimum(marker, under), -1).astype(np.int64)
    H, W = R.shape
    heap = [(-int(R[y, x]), y, x) for y, x in zip(*np.nonzero(region))]
    heapq.heapify(heap)
    while heap:
        v, y, x = heapq.heappop(heap)
        if -v < R[y, x]:
            continue
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < H and 0 <= nx < W and region[ny, nx]:
                c = min(int(under[ny, nx]), -v)
                if c > R[ny, nx]:
                    R[ny, nx] = c
                    heapq.heappush(heap, (-c, ny, nx))
    return np.maximum(R, 0)


def test_reconstruction_equals_the_priority_queue():
    raised = 0
    for H, W in ref.SIZES[:5]:
        for with_mask in (True, False):
            marker, under, mask = ref.recon_case(H, W, 2, with_mask=with_mask)
            want = ref.reconstruct_batch(marker, under, mask)
            for b in range(2):
                region = np.ones((H, W), bool) if mask is None else mask[b] != 0
                assert np.array_equal(want["out"][b], widest_paths(marker[b], under[b], region)), (H, W, with_mask, b)
            raised += int(want["raised"].sum())
            assert (want["status"] == 0).all()
    assert raised > 1000
    # by hand: one row, the marker 9 at the left end under the ceilings below; a wall (mask 0) stops it
    under = np.array([[9, 7, 8, 3, 5, 5]])
    marker = np.array([[9, 0, 0, 0, 0, 4]])
    assert ref.reconstruct(marker, under)["out"].tolist() == [[9, 7, 7, 3, 4, 4]]
    r = ref.reconstruct(marker, under, np.array([[1, 1, 0, 1, 1, 1]]))
    assert r["out"].tolist() == [[9, 7, 0, 3, 4, 4]] and r["raised"] == 3
    r = ref.reconstruct(np.array([[-1, ref.TOP + 1, ref.TOP]]), np.array([[5, 5, 5]]))
    assert r["status"] == 2 and r["out"].tolist() == [[5, 5, 5]] and r["raised"] == 2


@pytest.mark.parametrize("edge", ref.EDGES)
def test_seed_count_equals_the_count_by_dynamics(edge):
    for k, (name, m) in enumerate(all_masks()):
        region = m != 0
        for h in ref.HS:
            q, R1, R2 = maxima_of(k, h, edge)
            hq = ref.quanta(h, 0)[0]
            n = ndimage.label(region & (R2 < R1), ref.CROSS)[1]
            assert n == count_by_dynamics(q, region, hq), (name, h)
            assert n == ref.seeds(m, h, 0, edge)[1] or region.size > 66 * 66      # seeds() is these steps
            assert n >= ndimage.label(region, ref.CROSS)[1]                       # every component has a seed


def test_regional_maxima_equal_the_plateau_search():
    for k, (name, m) in enumerate(all_masks()):
        region = m != 0
        for h in (0, 2):
            q, R1, R2 = maxima_of(k, h, "ignore")
            assert np.array_equal(region & (R2 < R1), plateau_maxima(R1, region)), (name, h)
            hq = ref.quanta(h, 0)[0]
            assert (R1[region] <= q[region]).all() and (R1[region] >= q[region] - hq).all()


def two_discs():
    return ref.disc(64, 72, 30, 25, 12) | ref.disc(64, 72, 30, 45, 12)


def bridge():
    """Two discs of r = 12 joined by a bridge three pixels wide that swells to a disc of r = 4 half way."""
    m = ref.disc(64, 100, 30, 20, 12) | ref.disc(64, 100, 30, 80, 12) | ref.disc(64, 100, 30, 50, 4)
    m[29:32, 20:81] = True
    return m


def test_hand_worked_cases():
    n = lambda m, h, r=0.0, edge="ignore": ref.seeds(m, h, r, edge)[1]
    m = two_discs()
    q = ref.heights(m)
    assert q.max() == 192 and q[30, 35] == 112               # the peaks and the neck between them: 80 = 5 px apart
    assert [n(m, h) for h in (0, 2, 4.9, 5, 6)] == [2, 2, 2, 1, 1]
    ids = ref.seeds(m, 0)[0]
    assert ids[30, 25] == 1 and ids[30, 45] == 2 and (ids > 0).sum() == 2
    ids = ref.seeds(m, 2.0)[0]                               # a seed is the dome's top: what lies within h of the peak
    assert np.array_equal(ids == 1, (q >= 160) & (np.arange(72) < 35)) and np.array_equal(ids == 2, (q >= 160) & (np.arange(72) > 35))
    diag = ref.disc(64, 64, 25, 25, 12) | ref.disc(64, 64, 39, 39, 12)
    assert [n(diag, h) for h in (0, 0.5, 1, 2)] == [9, 3, 2, 2]
    assert [n(ref.disc(40, 40, 20, 20, 12), h) for h in ref.HS] == [1, 1, 1, 1]
    big_small = ref.disc(48, 56, 20, 20, 14) | ref.disc(48, 56, 20, 39, 6)
    assert [n(big_small, h) for h in (0, 1, 2, 3, 5)] == [2, 2, 2, 1, 1]
    full = np.ones((20, 30), bool)
    for h in ref.HS:
        ids, k = ref.seeds(full, h)                          # 'ignore': flat at H^2 + W^2, one plateau, the whole image
        assert k == 1 and (ids == 1).all()
        ids, k = ref.seeds(full, h, 0, "background")         # a ridge along the middle (rows 9 and 10, columns 9..20) and
        assert k == 1 and np.array_equal(ids > 0, ref.heights(full, "background") >= 160 - 16 * h)      # what lies within h of it
    assert ref.seeds(full, 2.0, 11, "background")[1] == 0 and ref.seeds(full, 2.0, 10, "background")[1] == 1
    one = np.ones((1, 1), bool)
    assert ref.distance2(one)[0, 0] == 2 and ref.distance2(one, "background")[0, 0] == 1
    assert ref.seeds(one, 2.0) == (np.ones((1, 1), np.int32), 1) and ref.seeds(np.zeros((1, 1)), 2.0)[1] == 0
    row = np.array([[1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1]])
    assert ref.distance2(row).tolist() == [[9, 4, 1, 0, 1, 4, 9, 4, 1, 0, 0, 1]]      # nothing above or below the row counts
    assert ref.distance2(row, "background").tolist() == [[1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1]]
    assert ref.seeds(row, 0)[0].tolist() == [[1, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 3]]
    assert ref.seeds(row, 0, 0, "background")[0].tolist() == [[1, 1, 1, 0, 2, 2, 2, 2, 2, 0, 0, 3]]
    m = bridge()
    ids, k = ref.seeds(m, 0.5)
    assert k == 3 and ids[30, 50] == 2                       # the swelling is a dome of its own
    ids, k = ref.seeds(m, 0.5, 6)
    assert k == 2 and ids[30, 50] == 0 and ids[30, 20] == 1 and ids[30, 80] == 2      # min_radius drops it, the cells' stay


def components_with(ids, region):
    """{component of the region: the number of distinct seeds in it}"""
    comp = ndimage.label(region, ref.CROSS)[0]
    pairs = np.unique(np.stack([comp[ids > 0], ids[ids > 0]]), axis=1)
    return dict(zip(*np.unique(pairs[0], return_counts=True)))


def check_busy(m, name):
    region = m != 0
    at2, at0 = ref.seeds(m, 2.0)[0], ref.seeds(m, 0)[0]
    per2, per0 = components_with(at2, region), components_with(at0, region)
    assert max(per2.values()) >= 2, name                                           # a component with at least two seeds
    assert any(per0[c] > per2[c] for c in per2), name                              # something merged
    assert ref.seeds(m, 2.0, 4)[1] < at2.max(), name                               # a seed that min_radius drops
    edge = np.zeros_like(region)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    assert (region & edge).any() and (ref.distance2(region) != ref.distance2(region, "background")).any(), name
    assert not np.array_equal(ref.seeds(m, 2.0)[0], ref.seeds(m, 2.0, 0, "background")[0]), name


def test_busy_inputs_hold_what_the_gpu_test_relies_on():
    seen = 0
    for H, W in ref.SIZES:
        for name, masks in ref.size_cases(H, W):
            if name.startswith("busy"):
                kinds = [m for m in masks if 0 < (m != 0).sum() < m.size]
                assert kinds, name
                for m in kinds if H * W <= 129 * 127 else kinds[:1]:
                    check_busy(m, (H, W, name))
                    seen += 1
            if name == "busy B4":
                assert not masks[0].any() and masks[2].all()
    assert seen >= 10


def test_the_gaussian_blob_mask():
    m = ref.blobs(130, 150)
    assert ndimage.label(m, ref.CROSS)[1] == 18
    assert [ref.seeds(m, h)[1] for h in (0, 1, 2, 3)] == [145, 40, 32, 28]
    assert ref.seeds(m, 2.0, 4)[1] == 25 and ref.seeds(m, 2.0, 0, "background")[1] == 31
    check_busy(m.astype(np.uint8), "blobs")


def test_the_serpentine():
    marker, under, mask = ref.serpentine()
    want = ref.reconstruct_batch(marker, under, mask)
    n = int((mask != 0).sum())
    assert n == 8420 and (want["out"][0][mask[0] != 0] == 500).all() and want["raised"][0] == n - 1
    assert ref.tiled_launches((0, 0), mask[0]) == 21 * 6 + 2 > 64      # 21 rows of the corridor, six tile borders each


def test_recon_cases_exercise_the_code():
    for H, W in ref.SIZES[2:]:
        marker, under, mask = ref.recon_case(H, W, 2)
        want = ref.reconstruct_batch(marker, under, mask)
        assert (want["raised"] > H * W // 20).all() and (mask == 0).any() and (want["out"][mask == 0] == 0).all()
