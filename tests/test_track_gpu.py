"""Linking cells across frames on the device (functions.link_frames -> unet_link_frames, functions.track_cells, tester.track)
against the numpy restatement tests/track_ref.py (pinned to hand-worked answers by tests/test_track_cpu.py).  Everything is
integers: every comparison is bit for bit.  Every pointer handed to the raw entry point is a poisoned guarded.Arena buffer."""
import numpy as np
import pytest
import torch

import guarded
import rand_ref
import track_ref as ref
from gpu_support import dev, hip, image, rejected  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 1), (2, 1, 65), (3, 5, 17), (2, 33, 31), (4, 64, 64), (3, 67, 130), (3, 200, 300), (2, 600, 900)]


def slots_for(n_pairs):
    """A power of two with room for twice the pairs."""
    return 1 << (2 * n_pairs + 1).bit_length()


def raw_link(dev, frm, to, n_max, slots):
    """unet_link_frames on guarded buffers (one buffer for both maps when they are one array): area, pred, pred_overlap, status
    as numpy int64."""
    import _hip
    a = guarded.Arena(dev)
    T, H, W = to.shape
    t = a.inp(torch.from_numpy(np.ascontiguousarray(to, np.int32)), "to")
    f = t if frm is to else a.inp(torch.from_numpy(np.ascontiguousarray(frm, np.int32)), "from")
    area, pred, over = (a.out((T, n_max + 1), torch.int32, k) for k in ("area", "pred", "pred_overlap"))
    status = a.out((T, 2), torch.int64, "status")
    scratch = a.scratch(_hip.lib().unet_link_frames_scratch_bytes(T, n_max, slots), "scratch")
    _hip.run("unet_link_frames", dev, a.ptr(f), a.ptr(t), T, H, W, n_max, slots, a.ptr(area), a.ptr(pred), a.ptr(over), a.ptr(status),
             a.ptr(scratch))
    a.verify(area, pred, over, status)                       # poison gone from every row, every guard intact
    return tuple(x.cpu().numpy().astype(np.int64) for x in (area, pred, over, status))


def same(got, want, what):
    for k, g, w in zip(("area", "pred", "pred_overlap", "status"), got, want):
        assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:4].tolist())


def check_raw(dev, frm, to, what, n_max=None):
    want = ref.links(frm, to, n_max)
    n_max = want[0].shape[1] - 1
    same(raw_link(dev, frm, to, n_max, slots_for(want[4])), want[:4], what)
    return want


@pytest.mark.parametrize("T,H,W", SHAPES)
def test_links_equal_the_restatement(dev, T, H, W):
    """One map against itself, with the exact id maximum and with a larger one; then two different maps."""
    m, other = ref.random_frames(0, T, H, W), ref.random_frames(1, T, H, W)
    want = check_raw(dev, m, m, "self")
    assert not want[3].any() and (T == 1 or H * W < 3 or want[1].any())
    check_raw(dev, m, m, "self, slack", n_max=int(m.max()) + 17)
    check_raw(dev, other, m, "from != to")
    if H * W >= 2000:
        assert (want[2][1:] > 1).sum() > 20 and want[4] > 100, "runs and many pairs"


def test_ties_go_to_the_smaller_id_in_both_orders(dev):
    for left, right in ((3, 8), (8, 3)):
        m = ref.tie_frames(left, right)
        want = check_raw(dev, m, m, (left, right))
        assert want[1][1, 1] == 3 and want[2][1, 1] == 4
    big = np.zeros((2, 40, 130), np.int32)                     # the same tie over thousands of pixels and many waves
    big[0, :, :65], big[0, :, 65:], big[1] = 70000, 5, 9
    for k in range(2):
        want = check_raw(dev, big, big, "big tie")
        assert want[1][1, 9] == 5 and want[2][1, 9] == 40 * 65
        big[0] = big[0, :, ::-1].copy()


def test_sparse_ids_above_16_bits(dev):
    m = ref.sparse_ids(33, 31)
    want = check_raw(dev, m, m, "sparse")
    assert want[0].shape == (2, 70002) and (want[1][1] > 65536).any() and len(np.nonzero(want[1][1])[0]) == 5


def test_ids_out_of_range_are_counted_and_ignored(dev):
    """Ids above n_max and negative ids: status[:, 0] counts the pixels of pair t that hold one in to[t] or from[t-1]; nothing
    else sees them."""
    m = ref.shifted_cells(7, 3, 40, 70, 9)
    n_max = int(m.max()) - 2
    m[0, 3, :9] = -1
    m[1, 5:8, 60:] = -(2 ** 31)
    m[2, 39, 69] = 1 << 24
    want = check_raw(dev, m, m, "bad ids", n_max=n_max)
    bad = (m < 0) | (m > n_max)
    assert bad[1].sum() >= 30 and want[3][:, 0].tolist() == [int(bad[0].sum()), int((bad[1] | bad[0]).sum()), int((bad[2] | bad[1]).sum())]
    assert want[0][1].sum() == 40 * 70 - want[3][1, 0]


def test_a_full_table_is_reported_and_link_frames_recovers(dev):
    import functions
    m = ref.shifted_cells(5, 6, 96, 120, 20)
    want = ref.links(m, m)
    n_max, slots = want[0].shape[1] - 1, 32
    assert want[4] > 2 * slots                               # the brute-force count of distinct (t, p, c): the table cannot hold them
    area, pred, over, status = raw_link(dev, m, m, n_max, slots)
    assert not status[:, 0].any() and status[:, 1].sum() > 0 and status[0, 1] == 0
    assert np.array_equal(area, want[0])                     # the areas do not go through the table
    assert (over <= want[2]).all()                           # a listed count holds no more than the pair's pixels
    t = torch.from_numpy(m).to(dev)
    for labels in (t, t.long()):
        got = functions.link_frames(labels, _table_slots=slots)
        assert all(g.dtype == np.int64 for g in got)
        same(got, want[:3], "doubled")
    same(functions.link_frames(t), want[:3], "default table")


def test_a_rejected_call_writes_nothing(dev, hip):
    a = guarded.Arena(dev)
    m = a.inp(torch.from_numpy(ref.random_frames(0, 2, 8, 8)), "maps")
    outs = [a.out((2, 41), torch.int32, k) for k in ("area", "pred", "pred_overlap")] + [a.out((2, 2), torch.int64, "status")]
    scratch = a.scratch(hip.lib().unet_link_frames_scratch_bytes(2, 40, 64), "scratch")
    L = hip.lib()

    def call(T=2, n_max=40, slots=64, null=None):
        ptrs = [None if k == null else a.ptr(o) for k, o in enumerate(outs)]
        return L.unet_link_frames(a.ptr(m), a.ptr(m), T, 8, 8, n_max, slots, *ptrs, a.ptr(scratch), None)

    for kw, words in (({"slots": 48}, b"power of two"), ({"slots": 0}, b"power of two"), ({"T": 0}, b"bad argument"),
                      ({"null": 1}, b"bad argument"), ({"null": 3}, b"bad argument"), ({"n_max": 1 << 24}, b"n_max"),
                      ({"n_max": -1}, b"n_max"), ({"T": 65536}, b"65535")):
        rejected(hip, call(**kw), a, *outs, scratch)
        assert words in L.unet_last_error(), kw
    assert call() == 0
    torch.cuda.synchronize()
    a.verify(*outs)


@pytest.fixture(scope="module")
def cells():
    return ref.shifted_cells(11, 4, 64, 80, 12, step=3)


def test_link_frames_with_reach(dev, cells):
    import functions
    for m in (cells, ref.drifting_discs()):
        t = torch.from_numpy(m).to(dev)
        plain = functions.link_frames(t)
        same(plain, ref.links(m, m)[:3], "plain")
        grown = rand_ref.grow_batch(m, [rand_ref.dist2(r) for r in (0, 1.5, 4)])
        for r in (0, 1.5, 4):
            got = functions.link_frames(t, reach=r)
            want = ref.links(grown[rand_ref.dist2(r)], m)
            assert not want[3].any()
            same(got, want[:3], r)
        same(functions.link_frames(t, reach=0), plain, "reach 0")
        assert (functions.link_frames(t, reach=4).pred_overlap >= plain.pred_overlap).all()


def test_errors_on_the_device(dev):
    import functions
    z = torch.zeros(2, 9, 7, dtype=torch.int32, device=dev)
    got = functions.link_frames(z)
    assert got.area.tolist() == [[63], [63]] and got.pred.tolist() == [[0], [0]]
    assert functions.link_frames(z[:1] + 2).area.tolist() == [[0, 0, 63]]
    neg = z.clone(); neg[1, 2, 3] = -1
    big = z.long(); big[0, 0, 0] = 1 << 24
    for f in (functions.link_frames, functions.track_cells):
        with pytest.raises(ValueError, match="negative"):
            f(neg)
        with pytest.raises(ValueError, match="2\\^24"):
            f(big)


def test_track_cells_equals_the_host_remap(dev):
    import functions
    for name, m in ref.sequences():
        for kw in ({}, {"reach": 3, "min_overlap": 0.3}, {"divisions": False}):
            src = m if "reach" not in kw else rand_ref.grow_batch(m, [9])[9]
            area, pred, over = ref.links(src, m)[:3]
            rules = {k: v for k, v in kw.items() if k != "reach"}
            table, track_of = ref.tracks(area, pred, over, **rules)
            maps, tracks = functions.track_cells(torch.from_numpy(m).to(dev), **kw)
            assert maps.dtype == torch.int32 and maps.is_cuda and maps.shape == m.shape
            assert np.array_equal(tracks.table, table) and np.array_equal(tracks.track_of, track_of), (name, kw)
            assert np.array_equal(maps.cpu().numpy(), ref.remap(m, track_of)), (name, kw)
            ref.check_structure(tracks.table, tracks.track_of, area)


def test_drifting_discs_keep_their_label_and_daughters_know_their_mother(dev):
    import functions
    shuffled, kept = ref.drifting_discs(0), ref.drifting_discs(0, shuffle=False)
    assert np.array_equal(shuffled != 0, kept != 0) and not np.array_equal(shuffled, kept)
    maps, tracks = functions.track_cells(torch.from_numpy(shuffled).to(dev))
    maps = maps.cpu().numpy()
    labels = [np.unique(maps[kept == k]) for k in range(1, 7)]
    assert all(len(l) == 1 for l in labels) and sorted(int(l[0]) for l in labels) == [1, 2, 3, 4, 5, 6]
    assert tracks.table.tolist() == [[k, 0, 4, 0] for k in range(1, 7)]
    m = ref.dividing_discs()
    maps, tracks = functions.track_cells(torch.from_numpy(m).to(dev))
    maps = maps.cpu().numpy()
    mother2, mother3 = int(maps[0, 20, 16]), int(maps[0, 20, 50])
    assert tracks.table[[int(maps[2, 20, 12]) - 1, int(maps[3, 20, 20]) - 1], 3].tolist() == [mother2] * 2
    assert tracks.table[[int(maps[2, 25, 45]) - 1, int(maps[3, 25, 55]) - 1, int(maps[2, 14, 50]) - 1], 3].tolist() == [mother3, mother3, 0]
    assert functions.track_cells(torch.from_numpy(m).to(dev), max_children=3)[1].table[int(maps[2, 14, 50]) - 1, 3] == mother3
    assert tracks.ctc_text().splitlines()[0] == "1 0 1 0"


def test_two_runs_give_identical_bytes(dev):
    import functions
    t = torch.from_numpy(ref.shifted_cells(5, 6, 96, 120, 20)).to(dev)
    a, b = functions.track_cells(t, reach=2), functions.track_cells(t, reach=2)
    assert torch.equal(a[0], b[0]) and a[1].table.tobytes() == b[1].table.tobytes() and a[1].track_of.tobytes() == b[1].track_of.tobytes()
    la, lb = functions.link_frames(t, _table_slots=64), functions.link_frames(t)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(la, lb))


def test_tester_track(dev):
    """A (3, 200, 260) random sequence through a default-initialised net and the smallest tile size: track is segment with
    return_instances, then track_cells.  The untrained net calls most of the image foreground; shape_split, handed through to
    segment, cuts that into cells."""
    import functions
    import network
    import tester
    torch.manual_seed(0)
    net = network.Unet().to(dev)
    x = torch.from_numpy(image(40, 3, 200, 260, blobs=12)).to(dev)
    kw = dict(tile_size=188, max_batch=64, shape_split=2.0)
    mask, maps, tracks = tester.track(net, x, reach=2, **kw)
    mask0, inst = tester.segment(net, x, return_instances=True, **kw)
    want_maps, want_tracks = functions.track_cells(inst, reach=2)
    print("%d foreground pixels, %d cells, %d tracks" % (int((mask != 0).sum()), int(inst.amax(dim=(1, 2)).sum()), len(tracks.table)))
    assert torch.equal(mask, mask0) and torch.equal(maps, want_maps) and np.array_equal(tracks.table, want_tracks.table)
    assert maps.shape == (3, 200, 260) and maps.dtype == torch.int32 and torch.equal(maps != 0, inst != 0)
    ref.check_structure(tracks.table, tracks.track_of, functions.link_frames(inst).area)



@pytest.mark.parametrize("slots", [None, 4])
@pytest.mark.parametrize("T,H,W", [(3, 5, 17), (3, 67, 130)])
def test_the_three_pair_fills_agree(dev, T, H, W, slots):
    """unet_partition_pairs, unet_link_frames and unet_instance_overlap fill their tables with one kernel: on the same maps the
    contingency table of frame t-1 (pred) against frame t (gt), cut down to p >= 1, must hold per c the link (largest count, the
    smallest p among equals) and per c the match (the p with 2 n > area).  slots = 4 makes every table overflow and double."""
    import _hip
    import functions
    m = ref.random_frames(2, T, H, W)
    m[m == 5] = 70001                                                  # one id above 16 bits
    n_max = int(m.max())
    assert n_max == 70001 and len(np.unique(m)) > 12
    t = torch.from_numpy(m).to(dev)
    gt, pred = t[1:].contiguous(), t[:-1].contiguous()
    pairs = functions.pair_table(pred, gt, _table_slots=slots)
    b, c, p, n = (x[pairs[2] >= 1] for x in pairs)
    assert len(n) > T and (n > 1).any()
    links = functions.link_frames(t, _table_slots=slots)
    # the table is sorted by (b, c, p): a stable sort by count descending keeps the smallest p first among equal counts
    order = np.lexsort((p, -n, c, b))
    first = np.ones(len(order), bool)
    first[1:] = (b[order][1:] != b[order][:-1]) | (c[order][1:] != c[order][:-1])
    best = order[first]
    want_pred, want_over = np.zeros((T, n_max + 1), np.int64), np.zeros((T, n_max + 1), np.int64)
    want_pred[b[best] + 1, c[best]], want_over[b[best] + 1, c[best]] = p[best], n[best]
    assert np.array_equal(links.pred, want_pred) and np.array_equal(links.pred_overlap, want_over)
    area = links.area[1:]
    half = 2 * n > area[b, c]
    want_match, want_inter = np.zeros((T - 1, n_max + 1), np.int64), np.zeros((T - 1, n_max + 1), np.int64)
    want_match[b[half], c[half]], want_inter[b[half], c[half]] = p[half], n[half]
    outs = [torch.empty(T - 1, n_max + 1, dtype=torch.int32, device=dev) for _ in range(4)]
    status = torch.empty(T - 1, 2, dtype=torch.int64, device=dev)
    table = slots_for(len(n))
    _hip.run("unet_instance_overlap", dev, _hip.ptr(gt), _hip.ptr(pred), T - 1, H, W, n_max, n_max, table, *(_hip.ptr(o) for o in outs),
             _hip.ptr(status), _hip.ptr(_hip.scratch("unet_instance_overlap", dev, T - 1, n_max, n_max, table)))
    area_gt, area_pred, match, inter = (o.cpu().numpy().astype(np.int64) for o in outs)
    assert not status.cpu().numpy().any()
    assert np.array_equal(area_gt, area) and np.array_equal(area_pred, links.area[:-1])
    assert np.array_equal(match, want_match) and np.array_equal(inter, want_inter) and (match > 0).sum() > T
    assert functions.seg_measure(pred, gt, _table_slots=slots).n_matched == (want_match[:, 1:] > 0).sum()
