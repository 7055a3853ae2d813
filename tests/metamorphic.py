"""Metamorphic relations of the exact image ops: what an op must answer on a changed input, stated as a relation of the op with
itself, so no reference is needed where the relation is used.  A plain module (imported like gpu_support, not a conftest);
importing it needs neither the library nor a device.

The definitions of the ops in OPS are geometric: they commute with the eight dihedral views (family D) and with translation
(family T), the images of a batch are independent (B), ids are names (R), and some ops have fixed points (F, the table FIXED).
tests/test_metamorphic_cpu.py proves every relation on the reference callables of the *_ref.py modules, and every exclusion, of a
family or of one field of a normal form under a family (Op.omits), by a counterexample on which the relation fails there; tests/test_metamorphic_gpu.py then holds the device ops to the same relations at
the seams of the kernels' decompositions.  Everything is compared bit for bit.

  view / unview, embed / extract, canon_labels, relabel     the transforms on planes [H,W] / [B,H,W]
  Tr                                                        how an input was changed, and how every kind of output comes back
  Op, OPS, FIXED                                            one entry per op: device wrapper, reference, normal form, families
  placements, seam_gaps                                     the placement plan of family T and its seam conditions
"""
import collections

import numpy as np

# ---- transforms on planes ---------------------------------------------------------------------------------------------------

VIEWS = tuple(range(8))


def view(a, v):
    """View v of [..,H,W]: transpose if v & 4, then flip the rows if v & 1, then the columns if v & 2."""
    a = np.swapaxes(np.asarray(a), -1, -2) if v & 4 else np.asarray(a)
    a = a[..., ::-1, :] if v & 1 else a
    return np.ascontiguousarray(a[..., ::-1] if v & 2 else a)


def unview(a, v):
    a = np.asarray(a)
    a = a[..., ::-1] if v & 2 else a
    a = a[..., ::-1, :] if v & 1 else a
    return np.ascontiguousarray(np.swapaxes(a, -1, -2) if v & 4 else a)


def compose(v, w):
    """The view u with view(view(a, v), w) == view(a, u), found on a probe without symmetry."""
    probe = np.arange(6).reshape(2, 3)
    got = view(view(probe, v), w)
    (u,) = [u for u in VIEWS if view(probe, u).shape == got.shape and np.array_equal(view(probe, u), got)]
    return u


def embed(scene, H, W, dy, dx, fill=0):
    """[..,h,w] -> [..,H,W]: the scene with its corner at (dy, dx), `fill` elsewhere."""
    scene = np.asarray(scene)
    h, w = scene.shape[-2:]
    assert 0 <= dy <= H - h and 0 <= dx <= W - w
    out = np.full(scene.shape[:-2] + (H, W), fill, scene.dtype)
    out[..., dy:dy + h, dx:dx + w] = scene
    return out


def extract(out, h, w, dy, dx):
    return np.ascontiguousarray(np.asarray(out)[..., dy:dy + h, dx:dx + w])


def canon_labels(lab):
    """Renumber the non-zero labels of [H,W] (of every image of [B,H,W]) 1..n by their first pixel in raster order; 0 stays."""
    lab = np.asarray(lab)
    if lab.ndim == 3:
        return np.stack([canon_labels(l) for l in lab]) if len(lab) else lab.astype(np.int64)
    vals, first, inv = np.unique(lab.ravel(), return_index=True, return_inverse=True)
    on = vals != 0
    rank = np.zeros(len(vals), np.int64)
    rank[np.flatnonzero(on)[np.argsort(first[on], kind="stable")]] = np.arange(1, int(on.sum()) + 1)
    return rank[inv].reshape(lab.shape)


def relabel(idmap, f):
    """f on every id of the map; f is a function on int64 arrays and must keep 0."""
    idmap = np.asarray(idmap)
    vals, inv = np.unique(idmap.ravel(), return_inverse=True)
    new = np.asarray(f(vals.astype(np.int64))).astype(np.int64)
    assert not new[vals == 0].any() and len(np.unique(new)) == len(new)
    return new[inv].reshape(idmap.shape).astype(idmap.dtype)


def order_map(i):
    return np.where(i > 0, 3 * i + 5, 0)


def top_map(top):
    """Order preserving, the largest id `top` of the map lands on 2^24 - 1."""
    return lambda i: np.where(i > 0, (1 << 24) - 1 - 3 * (top - i), 0)


def gap_permutation(ids, seed=0):
    """A permutation map of the ids present (an int64 array without 0) onto ids with gaps, 1, 7, 8 and 500 among them."""
    pool = [1, 7, 8, 500] + [13 + 5 * k for k in range(len(ids))]
    new = np.array(pool[:len(ids)], np.int64)
    np.random.RandomState(seed).shuffle(new)
    table = dict(zip(np.asarray(ids).tolist(), new.tolist()))
    return lambda i: np.array([table.get(int(v), 0) for v in np.asarray(i).ravel()], np.int64).reshape(np.shape(i))


class Tr:
    """How an input was changed, and how each kind of output comes back into the frame of the unchanged input.
    view: v, with (Hp, Wp) the shape of the changed input; shift: (dy, dx) with the scene's (h, w); ids: the pairs old -> new."""

    def __init__(self, v=0, shape=None, shift=None, scene=None, f=None, ids=None):
        self.v, self.shape, self.shift, self.scene = v, shape, shift, scene
        self.kind = "view" if v else "shift" if shift is not None else "relabel" if f is not None else None
        if f is not None:
            old = np.unique(np.concatenate([[0], np.asarray(ids).ravel()])).astype(np.int64)
            new = np.asarray(f(old)).astype(np.int64)
            order = np.argsort(new)
            self.new, self.old = new[order], old[order]

    def apply(self, x, id_inputs=()):
        """The changed input: x is a dict of planes [B,H,W]."""
        if self.kind == "view":
            return {k: view(a, self.v) for k, a in x.items()}
        if self.kind == "shift":
            H, W = self.shape
            return {k: embed(a, H, W, *self.shift) for k, a in x.items()}
        if self.kind == "relabel":
            back = dict(zip(self.old.tolist(), self.new.tolist()))
            return {k: relabel(a, lambda i: np.array([back[int(v)] for v in i], np.int64)) if k in id_inputs else a for k, a in x.items()}
        return dict(x)

    def plane(self, a):
        if self.kind == "view":
            return unview(a, self.v)
        if self.kind == "shift":
            return extract(a, *self.scene, *self.shift)
        return np.asarray(a)

    def ids(self, a):
        """Id values of the changed input -> the ids they were."""
        a = np.asarray(a).astype(np.int64)
        if self.kind != "relabel":
            return a
        at = np.searchsorted(self.new, a.ravel())
        assert np.array_equal(self.new[np.minimum(at, len(self.new) - 1)], a.ravel()), "an id the input did not hold"
        return self.old[at].reshape(a.shape)

    def points(self, y, x, corner=0):
        """Pixel coordinates (corner=0) or corner coordinates (corner=1: a pixel is [x, x+1] x [y, y+1]) of the changed frame."""
        y, x = np.asarray(y).astype(np.int64), np.asarray(x).astype(np.int64)
        if self.kind == "view":
            Hp, Wp = self.shape
            x = Wp - 1 + corner - x if self.v & 2 else x
            y = Hp - 1 + corner - y if self.v & 1 else y
            y, x = (x, y) if self.v & 4 else (y, x)
        elif self.kind == "shift":
            y, x = y - self.shift[0], x - self.shift[1]
        return y, x

    def boxes(self, box):
        """Half-open boxes (y0, x0, y1, x1) [.., 4] of present rows."""
        b = np.asarray(box).astype(np.int64)
        ya, xa = self.points(b[..., 0], b[..., 1], corner=1)
        yb, xb = self.points(b[..., 2], b[..., 3], corner=1)
        return np.stack([np.minimum(ya, yb), np.minimum(xa, xb), np.maximum(ya, yb), np.maximum(xa, xb)], axis=-1)

    def moments(self, m, n):
        """Raw sums (Sy, Sx, Syy, Sxx, Sxy) [.., 5] of n [..] pixels, by the affine rule."""
        sy, sx, syy, sxx, sxy = (np.asarray(m)[..., k].astype(np.int64) for k in range(5))
        n = np.asarray(n).astype(np.int64)

        def shifted(a, b):                                    # y -> y + a, x -> x + b
            return (sy + n * a, sx + n * b, syy + 2 * a * sy + n * a * a, sxx + 2 * b * sx + n * b * b, sxy + b * sy + a * sx + n * a * b)
        if self.kind == "view":
            Hp, Wp = self.shape
            if self.v & 2:                                    # x -> c - x
                c = Wp - 1
                sx, sxx, sxy = n * c - sx, n * c * c - 2 * c * sx + sxx, c * sy - sxy
            if self.v & 1:                                    # y -> c - y
                c = Hp - 1
                sy, syy, sxy = n * c - sy, n * c * c - 2 * c * sy + syy, c * sx - sxy
            if self.v & 4:
                sy, sx, syy, sxx = sx, sy, sxx, syy
        elif self.kind == "shift":
            sy, sx, syy, sxx, sxy = shifted(-self.shift[0], -self.shift[1])
        return np.stack([sy, sx, syy, sxx, sxy], axis=-1)


def per_id(tr, present, cols, skip0=False):
    """Per-id rows [B,N,..] -> rows over the (image, id) pairs present, sorted by (image, the id it was); absent rows must be 0."""
    present = np.asarray(present).astype(bool)
    b, i = np.nonzero(present)
    if skip0:
        b, i = b[i > 0], i[i > 0]
    was = tr.ids(i)
    order = np.lexsort((was, b))
    out = {"table:id": np.stack([b[order], was[order]], axis=1)}
    for k, c in cols.items():
        c = np.asarray(c)
        assert not c[~present].any(), "%s: a row of an absent id is not 0" % k
        rows = c[b, i][order]
        out["table:" + k] = np.concatenate([b[order][:, None], rows.reshape(len(rows), int(np.prod(rows.shape[1:])))], axis=1)
    return out


def pick(o, b):
    """Image b of a normal form: planes and per-image words by index, tables by their image column (then 0)."""
    out = {}
    for k, a in o.items():
        if k.startswith("batch:"):                            # a word of the whole batch has no image b: relation_B sums the integer ones
            continue
        if k.startswith("table:"):
            rows = a[a[:, 0] == b].copy()
            rows[:, 0] = 0
            out[k] = rows
        else:
            out[k] = a[b:b + 1]
    return out


def same(a, b):
    """None if the two normal forms are equal bit for bit, else the first key that differs."""
    if sorted(a) != sorted(b):
        return "keys %s / %s" % (sorted(a), sorted(b))
    for k in sorted(a):
        u, v = np.asarray(a[k]), np.asarray(b[k])
        if u.shape != v.shape or not np.array_equal(u, v, equal_nan=u.dtype.kind == "f" and v.dtype.kind == "f"):
            return k
    return None


# ---- the ops ----------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()     # a copy: a view of a one-row image keeps a negative stride


def _np(t):
    return t.cpu().numpy()


def _F():
    import functions
    return functions


HOLDS = "holds"
Excluded = collections.namedtuple("Excluded", "reason counterexample")     # counterexample: the name of a function of COUNTER
Op = collections.namedtuple("Op", "name inputs id_inputs gpu ref normal families relabel two_class lattice omits")
OPS = collections.OrderedDict()
COUNTER = {}


def _op(name, inputs, gpu, ref, normal, *, relabel=None, id_inputs=(), excluded=None, two_class=False, lattice=1, omits=None):
    """omits: {family: {field: Excluded}}, the fields of the normal form that a family that otherwise holds does not carry, each
    with a counterexample on which that field breaks the relation on the reference; they count as exclusions of (op, family)."""
    fam = {"D": HOLDS, "T": HOLDS, "B": HOLDS}
    if relabel:
        fam["R"] = HOLDS
    fam.update(excluded or {})
    OPS[name] = Op(name, inputs, id_inputs, gpu, ref, normal, fam, relabel, two_class, lattice, omits or {})


def run(name, x, backend, tr=None, **kw):
    """The normal form of op `name` on the input x (a dict of planes [B,H,W]) that was changed by tr: backend 'gpu' is the
    wrapper on the device, 'ref' the reference callable, a function stands in for either (a deliberately broken op)."""
    op = OPS[name]
    fn = op.gpu if backend == "gpu" else op.ref if backend == "ref" else backend
    return op.normal(fn({k: x[k] for k in op.inputs}, **kw), tr or Tr())


def _labels(conn):
    import clean_ref

    def gpu(x):
        lab, n = _F().label_cells(_dev(x["mask"]), connectivity=conn)
        return {"lab": _np(lab), "n": _np(n)}

    def ref(x):
        lab, n = clean_ref.label_batch(x["mask"], conn)
        return {"lab": lab, "n": n}
    return gpu, ref, lambda o, tr: {"lab": canon_labels(tr.plane(o["lab"])), "n": np.asarray(o["n"])}


def _clean(conn, only=None):
    import clean_ref

    def params(kw):
        if only == "fill":
            return dict(fill_holes=True, max_hole_area=kw.get("max_hole_area"), min_area=0, drop_border=False)
        if only == "small":
            return dict(fill_holes=False, max_hole_area=None, min_area=kw.get("min_area", 4), drop_border=False)
        return dict(fill_holes=True, max_hole_area=None, min_area=kw.get("min_area", 4), drop_border=kw.get("drop_border", True))

    def gpu(x, **kw):
        F, p, m = _F(), params(kw), _dev(x["mask"])
        if only == "fill":
            return {"out": _np(F.fill_holes(m, p["max_hole_area"], conn))}
        if only == "small":
            return {"out": _np(F.remove_small(m, p["min_area"], conn))}
        out, info, action = F.clean_mask(m, connectivity=conn, return_info=True, return_action=True, **p)
        return {"out": _np(out), "action": _np(action), "info": np.stack(list(info), axis=1)}

    def ref(x, **kw):
        r = clean_ref.clean_batch(x["mask"], connectivity=conn, **params(kw))
        return {"out": r["out"]} if only else r
    return gpu, ref, lambda o, tr: {k: (v if k == "info" else tr.plane(v)) for k, v in o.items()}


def _distance(edge):
    import shape_ref

    def gpu(x):
        return {"d2": _np(_F().distance_map(_dev(x["mask"]), edge=edge))}

    def ref(x):
        return {"d2": np.stack([shape_ref.distance2(m, edge) for m in x["mask"]])}
    return gpu, ref, lambda o, tr: {"d2": tr.plane(o["d2"])}


def _reconstruct(conn):
    import conn_ref

    def gpu(x):
        R, info = _F().reconstruct(_dev(x["marker"]), _dev(x["under"]), connectivity=conn)
        return {"R": _np(R), "raised": info.raised}

    def ref(x):
        r = conn_ref.reconstruct_batch(x["marker"], x["under"], None, conn)
        return {"R": r["out"], "raised": r["raised"]}
    return gpu, ref, lambda o, tr: {"R": tr.plane(o["R"]), "raised": np.asarray(o["raised"])}


def _shape_seeds(conn):
    import conn_ref

    def gpu(x, h=1.0):
        s, n = _F().shape_seeds(_dev(x["mask"]), h, edge="ignore", connectivity=conn)
        return {"seeds": _np(s), "n": _np(n)}

    def ref(x, h=1.0):
        s, n = conn_ref.seeds_batch(x["mask"], h, 0.0, "ignore", conn)
        return {"seeds": s, "n": n}
    return gpu, ref, lambda o, tr: {"seeds": canon_labels(tr.plane(o["seeds"])), "n": np.asarray(o["n"])}


def _split(conn):
    import conn_ref

    def gpu(x, max_steps=None):
        lab, info, dist = _F().split_cells(_dev(x["seeds"]), _dev(x["region"]), max_steps=max_steps, return_distance=True, connectivity=conn)
        return {"labels": _np(lab), "dist": _np(dist), "words": np.stack([info.seeds_outside, info.unreached, info.max_distance], axis=1)}

    def ref(x, max_steps=None):
        r = conn_ref.grow_batch(x["seeds"], x["region"], max_steps, conn)
        return {"labels": r["out"], "dist": r["dist"], "words": np.stack([r["seeds_outside"], r["unreached"], r["max_dist"]], axis=1)}
    return gpu, ref, lambda o, tr: {"labels": tr.ids(tr.plane(o["labels"])), "dist": tr.plane(o["dist"]), "words": o["words"]}


def _watershed(conn):
    import conn_ref

    def gpu(x):
        lab, info, lev, dist = _F().watershed(_dev(x["seeds"]), _dev(x["image"]), mask=_dev(x["region"]), return_levels=True, connectivity=conn)
        return {"labels": _np(lab), "level": _np(lev), "dist": _np(dist),
                "words": np.stack([info.seeds_outside, info.unreached, info.max_level], axis=1)}

    def ref(x):
        r = conn_ref.flood_batch(x["seeds"], x["image"], x["region"], None, None, conn)
        return {"labels": r["out"], "level": r["pass_level"], "dist": r["dist"],
                "words": np.stack([r["seeds_outside"], r["unreached"], r["max_level"]], axis=1)}
    return gpu, ref, lambda o, tr: {"labels": tr.ids(tr.plane(o["labels"])), "level": tr.plane(o["level"]), "dist": tr.plane(o["dist"]),
                                    "words": o["words"]}


def _grow():
    import rand_ref

    def gpu(x, max_distance=None):
        return {"out": _np(_F().grow_cells(_dev(x["ids"]), max_distance))}

    def ref(x, max_distance=None):
        d2 = rand_ref.dist2(max_distance)
        return {"out": rand_ref.grow_batch(x["ids"], [d2])[d2]}
    return gpu, ref, lambda o, tr: {"out": tr.ids(tr.plane(o["out"]))}


SUM_ROWS = ("area", "frame", "open", "contact", "v_sum", "v_sum2", "v_min", "v_max")


def _sums():
    import measure_ref

    def gpu(x):
        s = _F().cell_sums(_dev(x["ids"]), _dev(x["image16"]))
        return {k: _np(getattr(s, k)) for k in s._fields}

    def ref(x):
        return measure_ref.sums_batch(x["ids"], x["image16"])

    def normal(o, tr):
        cols = {k: o[k] for k in SUM_ROWS}
        on = np.asarray(o["present"]).astype(bool)
        cols["bbox"] = np.where(on[..., None], tr.boxes(o["bbox"]), 0)
        cols["moments"] = np.where(on[..., None], tr.moments(o["moments"], o["area"]), 0)
        return per_id(tr, on, cols, skip0=tr.kind == "shift")               # the background row belongs to the canvas
    return gpu, ref, normal


def _hulls():
    import hull_ref

    def gpu(x):
        h = _F().cell_hulls(_dev(x["ids"]))
        return {"n_vertices": _np(h.n_vertices), "area2": _np(h.area2), "feret_max2": _np(h.feret_max2),
                "width": np.stack([_np(h.width_cross), _np(h.width_len2)], axis=-1), "offset": _np(h.offset), "vertices": _np(h.vertices)}

    def ref(x):
        return hull_ref.hulls(x["ids"])

    def normal(o, tr):
        nv = np.asarray(o["n_vertices"]).astype(np.int64)
        B, N = nv.shape
        out = per_id(tr, nv > 0, {k: o[k] for k in ("n_vertices", "area2", "feret_max2", "width")})
        rows = []
        for b, i in zip(*np.nonzero(nv)):
            s = 2 * int(o["offset"][b * N + i])
            v = np.asarray(o["vertices"])[s:s + nv[b, i]]
            assert not np.asarray(o["vertices"])[s + nv[b, i]:2 * int(o["offset"][b * N + i + 1])].any()
            y, x = tr.points(v[:, 1], v[:, 0], corner=1)
            rows.append(np.stack([np.full(len(v), b), np.full(len(v), int(tr.ids(i))), x, y], axis=1))
        rows = np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)
        out["table:vertices"] = rows[np.lexsort(rows.T[::-1])]               # as a set: sorted by (image, id, x, y)
        return out
    return gpu, ref, normal


def _pairs_sorted(tr, b, i, j, n, unordered):
    i, j = tr.ids(i), tr.ids(j)
    if unordered:
        i, j = np.minimum(i, j), np.maximum(i, j)
    rows = np.stack([np.asarray(b).astype(np.int64), i, j, np.asarray(n).astype(np.int64)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def _neighbours():
    import hull_ref

    def gpu(x):
        return dict(zip("bijn", _F().cell_neighbours(_dev(x["ids"]))))

    def ref(x):
        return dict(zip("bijn", hull_ref.contacts(x["ids"])))
    return gpu, ref, lambda o, tr: {"table:contacts": _pairs_sorted(tr, o["b"], o["i"], o["j"], o["n"], True)}


def keep_rule(ids):
    """bool [B, n_max+1]: keep the cells of even area, a decision that follows a cell through every view, shift and renaming."""
    ids = np.asarray(ids)
    N = int(ids.max()) + 1
    area = np.stack([np.bincount(i.ravel(), minlength=N) for i in ids])
    return (area > 0) & (area % 2 == 0)


def _select():
    import measure_ref

    def gpu(x):
        return {"out": _np(_F().select_cells(_dev(x["ids"]), _dev(keep_rule(x["ids"]))))}

    def ref(x):
        return {"out": measure_ref.select(x["ids"], keep_rule(x["ids"]))}
    return gpu, ref, lambda o, tr: {"out": tr.ids(tr.plane(o["out"]))}


def _seg():
    import instances_ref

    words = ("per_image", "jaccard", "seg", "jaccard_sum", "n_gt", "n_matched", "n_pred")

    def gpu(x):
        s = _F().seg_measure(_dev(x["ids2"]), _dev(x["ids"]))
        return {k: getattr(s, k) for k in words}

    def ref(x):
        s = instances_ref.seg(x["ids"], x["ids2"])
        return {k: s[k] for k in words}

    def normal(o, tr):
        rows = [np.stack([np.full(len(j), float(b)), np.sort(j)], axis=1) for b, j in enumerate(o["jaccard"])]
        return {"table:jaccard": np.concatenate(rows) if rows else np.zeros((0, 2)),      # the J of an image as a multiset
                "per_image": np.asarray(o["per_image"]), "batch:seg": np.float64(o["seg"]), "batch:jaccard_sum": np.float64(o["jaccard_sum"]),
                "batch:counts": np.array([o["n_gt"], o["n_matched"], o["n_pred"]], np.int64)}
    return gpu, ref, normal


RAND_WORDS = ("rand_split", "rand_merge", "v_rand", "rand_error", "info_split", "info_merge", "v_info", "voi_split", "voi_merge")
RAND_INTS = ("N", "S_pair", "S_pred", "S_gt", "c")


def _rand():
    import rand_ref

    def gpu(x):
        F, p, g = _F(), _dev(x["ids2"]), _dev(x["ids"])
        s = F.rand_scores(p, g)
        return {"table": F.pair_table(p, g), "scores": np.stack([getattr(s, k) for k in RAND_WORDS], axis=1),
                "ints": np.stack([getattr(s, k) for k in RAND_INTS], axis=1)}

    def ref(x):
        s = rand_ref.scores(x["ids2"], x["ids"])
        return {"table": rand_ref.pairs(x["ids2"], x["ids"]), "scores": np.stack([s[k] for k in RAND_WORDS], axis=1),
                "ints": np.stack([s[k] for k in RAND_INTS], axis=1)}
    return gpu, ref, lambda o, tr: {"table:pairs": _pairs_sorted(tr, *o["table"], False), "scores": o["scores"], "ints": o["ints"]}


def _links():
    import track_ref

    def frames(x):
        """Image b is the pair of frames (ids2[b], ids[b]); the time-lapse alternates them and only the links inside a pair count."""
        return np.stack([x["ids2"], x["ids"]], axis=1).reshape((-1,) + x["ids"].shape[1:])

    def gpu(x):
        area, pred, over = _F().link_frames(_dev(frames(x)))
        return {"area": area[1::2], "pred": pred[1::2], "overlap": over[1::2]}

    def ref(x):
        f = frames(x)
        area, pred, over = track_ref.links(f, f)[:3]
        return {"area": area[1::2], "pred": pred[1::2], "overlap": over[1::2]}

    def normal(o, tr):
        return per_id(tr, np.asarray(o["area"]) > 0, {"area": o["area"], "pred": tr.ids(o["pred"]), "overlap": o["overlap"]}, skip0=True)
    return gpu, ref, normal


SURFACE = dict(tolerances=(1.0, 2.5), percentile=95)
SURFACE_VARIANTS = ((4, "background"), (8, "ignore"))


def sum_in_raster_order(d2):
    """The fp64 sum of sqrt(d2) over the contour pixels of a plane (d2 >= 0) the way unet_hip.h states it: rounded, in a fixed order
    that follows the raster.  Per 256-pixel chunk of a row a tree over the 64 lanes of each of four waves, the waves in order,
    then the chunks in raster order.  (boundary_ref's math.fsum is the exact sum: it cannot tell whether an order matters.  The
    tree inside a chunk is this restatement's choice; it stands for the kind of order, not for the device's bits.)"""
    d2 = np.asarray(d2)
    H, W = d2.shape
    total = np.float64(0.0)
    for y in range(H):
        for x0 in range(0, W, 256):
            c = d2[y, x0:x0 + 256]
            v = np.zeros(256)
            v[:len(c)] = np.where(c >= 0, np.sqrt(np.maximum(c, 0).astype(np.float64)), 0.0)
            w = v.reshape(4, 64)
            k = 32
            while k:
                w = w[:, :k] + w[:, k:2 * k]
                k //= 2
            total = total + (((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])
    return total


def _tagged(variants, make):
    """One op of several settings: every field of the normal form carries the setting's tag."""
    parts = [("[%s]" % ",".join(str(v) for v in var), make(*var)) for var in variants]

    def gpu(x):
        return {tag: g(x) for tag, (g, _, _) in parts}

    def ref(x):
        return {tag: r(x) for tag, (_, r, _) in parts}

    def normal(o, tr):
        return {k + tag: v for tag, (_, _, n) in parts for k, v in n(o[tag], tr).items()}
    return gpu, ref, normal


def _boundary(conn, edge):
    import boundary_ref

    def gpu(x):
        F, p, g = _F(), _dev(x["mask2"]), _dev(x["mask"])
        s = F.surface_sums(p, g, connectivity=conn, edge=edge, return_maps=True, **SURFACE)
        rec = _np(s.record)
        return {"contour": _np(F.mask_boundary(g, connectivity=conn, edge=edge)), "d2_pred": _np(s.d2_pred), "d2_gt": _np(s.d2_gt),
                "words": rec[..., :9], "sum": np.ascontiguousarray(rec[..., 9]).view(np.float64)}

    def ref(x):
        per = [boundary_ref.surface(p, g, connectivity=conn, edge=edge, **SURFACE) for p, g in zip(x["mask2"], x["mask"])]
        return {"contour": np.stack([boundary_ref.contour(boundary_ref.region(g), conn, edge) for g in x["mask"]]),
                "d2_pred": np.stack([s["d2"][0] for s in per]), "d2_gt": np.stack([s["d2"][1] for s in per]),
                "words": np.array([[r[:9] for r in s["record"]] for s in per], np.int64),
                "sum": np.array([[sum_in_raster_order(d) if r[0] and r[9] else 0.0 for r, d in zip(s["record"], s["d2"])] for s in per], np.float64)}

    def normal(o, tr):
        out = {k: tr.plane(o[k]) for k in ("contour", "d2_pred", "d2_gt")}
        out.update(words=np.asarray(o["words"]), sum=np.asarray(o["sum"]))
        return out
    return gpu, ref, normal


def _weighted():
    import weighted_map_ref

    def gpu(x):
        w, n = _F().weighted_map(_dev(x["mask"].astype(np.int64)), return_objects=True)
        return {"w": _np(w), "n": _np(n)}

    def ref(x):
        w, n = weighted_map_ref.weighted_map_batch(x["mask"].astype(np.int64))
        return {"w": w, "n": n}
    return gpu, ref, lambda o, tr: {"w": tr.plane(np.ascontiguousarray(o["w"], np.float32).view(np.int32)), "n": np.asarray(o["n"])}


def _carve():
    import prepare_ref

    def gpu(x):
        import data
        ids = _dev(x["ids"])
        gt, edges = data.preprocess_gt(ids)
        return {"gt": _np(gt), "edges": _np(edges), "bin": _np(data.binary_target(ids))}

    def ref(x):
        gt, edges, binary, _ = prepare_ref.carve_batch(x["ids"], 4)
        return {"gt": gt, "edges": edges, "bin": binary}
    return gpu, ref, lambda o, tr: {k: tr.plane(v) for k, v in o.items()}


def _warp(conn):
    import warp_ref

    def gpu(x):
        w, c = _F().warp_labels(_dev(x["mask"]), _dev(x["mask2"]), connectivity=conn)
        return {"warped": _np(w), "mismatch_map": _np(c.mismatch_map), "words": np.stack([c.mismatch, c.mismatch_before, c.flips], axis=1)}

    def ref(x):
        r = warp_ref.warp_batch(x["mask"], x["mask2"], connectivity=conn)
        return {"warped": r["warped"], "mismatch_map": r["mismatch_map"], "words": np.stack([r["mismatch"], r["mismatch_before"], r["flips"]], axis=1)}
    return gpu, ref, lambda o, tr: {"warped": tr.plane(o["warped"]), "mismatch_map": tr.plane(o["mismatch_map"]) != 0, "words": o["words"]}


def warp_counterexample():
    """Inputs [1,8,8] of warp_labels on which the order of the four passes shows: the passes are named by the parity of the absolute
    row and column, (y & 1) * 2 + (x & 1), so a transpose swaps passes 1 and 2 and a shift by an odd amount renames them all."""
    gt, pred = np.zeros((1, 8, 8), np.uint8), np.zeros((1, 8, 8), np.uint8)
    gt[0, 2:6, 2:6] = [[0, 1, 1, 1], [0, 0, 0, 1], [1, 1, 0, 0], [1, 1, 1, 0]]
    pred[0, 2:6, 2:6] = [[1, 0, 0, 1], [1, 0, 1, 0], [1, 0, 1, 0], [0, 0, 1, 0]]
    return {"mask": gt, "mask2": pred}


def surface_counterexample():
    """Inputs [1,6,12] of surface_sums whose distances are many different square roots: their rounded sum shows its order."""
    gt, pred = np.zeros((1, 6, 12), np.uint8), np.zeros((1, 6, 12), np.uint8)
    pred[0, 1:5, 1:11] = [[1, 1, 1, 1, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 0, 0, 1, 1, 0, 1], [1, 1, 1, 1, 0, 1, 0, 1, 0, 0], [0, 1, 1, 0, 0, 0, 1, 1, 1, 0]]
    gt[0, 1:5, 1:11] = [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1, 0, 0], [1, 0, 1, 0, 1, 0, 0, 0, 1, 1]]
    return {"mask": gt, "mask2": pred}


SURFACE_COUNTER_VIEWS, SURFACE_COUNTER_PLAN = VIEWS[1:], [(0, 0), (1, 60), (0, 58), (2, 30)]

# Each runs the relation of the family on a scene where it fails on the reference; field: the omitted field to compare all the same.
COUNTER["warp_view"] = lambda name, backend, field=None: relation_D(name, warp_counterexample(), backend, views=(4,))
COUNTER["surface_sum_view"] = lambda name, backend, field: relation_D(name, surface_counterexample(), backend, SURFACE_COUNTER_VIEWS, include=field)
COUNTER["surface_sum_shift"] = lambda name, backend, field: relation_T(name, surface_counterexample(), backend, (8, 80), SURFACE_COUNTER_PLAN,
                                                                      include=field)


def _seg_mean_renamed(name, backend, field):
    x = inputs_of(*composed_scene())
    ids = _all_ids(OPS[name], x)
    relation_R(name, x, backend, gap_permutation(ids[ids > 0], 2), include=field)


COUNTER["seg_mean_renamed"] = _seg_mean_renamed


def _build():
    for conn in (4, 8):
        _op("label_cells[%d]" % conn, ("mask",), *_labels(conn))
        _op("clean_mask[%d]" % conn, ("mask",), *_clean(conn))
        _op("fill_holes[%d]" % conn, ("mask",), *_clean(conn, "fill"))
        _op("remove_small[%d]" % conn, ("mask",), *_clean(conn, "small"))
    for edge in ("ignore", "background"):
        _op("distance_map[%s]" % edge, ("mask",), *_distance(edge))
    for conn in (4, 8):
        _op("reconstruct[%d]" % conn, ("marker", "under"), *_reconstruct(conn))
    _op("shape_seeds[4]", ("mask",), *_shape_seeds(4))
    _op("shape_seeds[8]", ("mask",), *_shape_seeds(8))
    for conn in (4, 8):
        _op("split_cells[%d]" % conn, ("seeds", "region"), *_split(conn), relabel="order", id_inputs=("seeds",))
        _op("watershed[%d]" % conn, ("seeds", "image", "region"), *_watershed(conn), relabel="order", id_inputs=("seeds",))
    _op("grow_cells", ("ids",), *_grow(), relabel="order", id_inputs=("ids",))
    _op("cell_sums", ("ids", "image16"), *_sums(), relabel="perm", id_inputs=("ids",))
    _op("cell_hulls", ("ids",), *_hulls(), relabel="perm", id_inputs=("ids",))
    _op("cell_neighbours", ("ids",), *_neighbours(), relabel="perm", id_inputs=("ids",))
    _op("select_cells", ("ids",), *_select(), relabel="perm", id_inputs=("ids",))
    mean = "a rounded float sum over the cells in increasing id order: a permutation of the ids changes the order"
    _op("seg_measure", ("ids", "ids2"), *_seg(), relabel="perm", id_inputs=("ids", "ids2"),
        omits={"R": {k: Excluded(mean, "seg_mean_renamed") for k in ("per_image", "batch:seg", "batch:jaccard_sum")}})
    _op("rand_scores", ("ids", "ids2"), *_rand(), relabel="perm", id_inputs=("ids", "ids2"))
    _op("link_frames", ("ids", "ids2"), *_links(), relabel="order", id_inputs=("ids", "ids2"))
    order = "the fp64 sum of sqrt(d2) is rounded in a fixed order that follows the raster (unet_hip.h): a %s changes the order"
    sums = ["sum[%d,%s]" % v for v in SURFACE_VARIANTS]
    _op("surface_sums", ("mask", "mask2"), *_tagged(SURFACE_VARIANTS, _boundary),
        omits={"D": {k: Excluded(order % "view", "surface_sum_view") for k in sums},
               "T": {k: Excluded(order % "shift", "surface_sum_shift") for k in sums}})
    _op("warp_labels", ("mask", "mask2"), *_tagged(((4,), (8,)), _warp), lattice=2, excluded={"D": Excluded(
        "the four passes of a sweep are named by the parity of the absolute row and column: a view renames them", "warp_view")})
    _op("weighted_map", ("mask",), *_weighted(), two_class=True)
    _op("carve_borders", ("ids",), *_carve())


_build()


# ---- fixed points (family F) ------------------------------------------------------------------------------------------------
# Each takes call(name, x, **kw) -> normal form (of the device or of the reference) and the inputs of a scene, and asserts.

def _f_clean(call, x):
    for name in ("clean_mask[4]", "clean_mask[8]"):
        a = call(name, x)
        b = call(name, {"mask": a["out"]})
        assert same({"out": a["out"]}, {"out": b["out"]}) is None
        assert not b["info"][:, :6].any() and np.array_equal(b["info"][:, 6], a["info"][:, 6])
        assert np.array_equal(b["action"], (a["out"] != 0).astype(np.uint8))


def _f_fill(call, x):
    for name in ("fill_holes[4]", "fill_holes[8]"):
        a = call(name, x)
        assert same(a, call(name, {"mask": a["out"]})) is None


def _f_label(call, x):
    for name in ("label_cells[4]", "label_cells[8]"):
        a = call(name, x)
        assert same(a, call(name, {"mask": (a["lab"] > 0).astype(np.uint8)})) is None


def _f_reconstruct(call, x):
    for name in ("reconstruct[4]", "reconstruct[8]"):
        a = call(name, x)
        b = call(name, {"marker": a["R"].astype(np.int32), "under": x["under"]})
        assert np.array_equal(a["R"], b["R"]) and not b["raised"].any()


def _f_grow(call, x):
    assert np.array_equal(call("grow_cells", x, max_distance=0)["out"], x["ids"])


def _f_split(call, x):
    for name in ("split_cells[4]", "split_cells[8]"):
        a = call(name, x)
        b = call(name, {"seeds": a["labels"].astype(np.int32), "region": x["region"]})
        assert np.array_equal(a["labels"], b["labels"]) and not b["dist"][b["labels"] > 0].any()


def _f_distance(call, x):
    for name in ("distance_map[ignore]", "distance_map[background]"):
        assert np.array_equal(call(name, x)["d2"] == 0, x["mask"] == 0)


def _f_surface(call, x):
    every = call("surface_sums", {"mask": x["mask"], "mask2": x["mask"]})
    for tag in ("[4,background]", "[8,ignore]"):
        a = {k[:-len(tag)]: v for k, v in every.items() if k.endswith(tag)}
        n = a["contour"].reshape(len(a["contour"]), -1).sum(axis=1)
        w = a["words"]
        assert np.array_equal(w[:, 0, 0], n) and np.array_equal(w[:, 1, 0], n)
        assert not w[:, :, 1:4].any() and not a["sum"].any()                # max, lo, hi and the sum: all distances are 0
        assert (w[:, :, 5:7] == n[:, None, None]).all()                    # full NSD at both tolerances
        assert np.array_equal(a["d2_pred"], np.where(a["contour"] != 0, 0, -1)) and np.array_equal(a["d2_pred"], a["d2_gt"])


def _f_scores(call, x):
    both = {"ids": x["ids"], "ids2": x["ids"]}
    g = call("seg_measure", both)
    j, n = g["table:jaccard"], g["batch:counts"]
    assert len(j) and (j[:, 1] == 1.0).all() and n[0] == n[1] == n[2] == len(j)
    assert g["batch:seg"] == 1.0 and g["batch:jaccard_sum"] == len(j)
    assert all(v == 1.0 or (np.isnan(v) and not (j[:, 0] == b).any()) for b, v in enumerate(g["per_image"]))
    r = call("rand_scores", both)
    s = dict(zip(RAND_WORDS, r["scores"].T))
    for k in ("rand_split", "rand_merge", "v_rand"):
        assert (s[k] == 1.0).all(), k
    assert not s["rand_error"].any() and (r["table:pairs"][:, 1] == r["table:pairs"][:, 2]).all()


def _f_warp(call, x):
    a = call("warp_labels", {"mask": x["mask"], "mask2": x["mask"]})
    for tag in ("[4]", "[8]"):
        assert np.array_equal(a["warped" + tag], x["mask"] != 0) and not a["words" + tag].any() and not a["mismatch_map" + tag].any()


FIXED = collections.OrderedDict([
    ("clean_mask", (_f_clean, ("clean_mask[4]", "clean_mask[8]"))),
    ("fill_holes", (_f_fill, ("fill_holes[4]", "fill_holes[8]"))),
    ("label_cells", (_f_label, ("label_cells[4]", "label_cells[8]"))),
    ("reconstruct", (_f_reconstruct, ("reconstruct[4]", "reconstruct[8]"))),
    ("grow_cells", (_f_grow, ("grow_cells",))),
    ("split_cells", (_f_split, ("split_cells[4]", "split_cells[8]"))),
    ("distance_map", (_f_distance, ("distance_map[ignore]", "distance_map[background]"))),
    ("surface_sums", (_f_surface, ("surface_sums",))),
    ("scores", (_f_scores, ("seg_measure", "rand_scores"))),
    ("warp_labels", (_f_warp, ("warp_labels",))),
])


def families(name):
    """The families of an op that hold, F included where FIXED names the op."""
    got = {f for f, s in OPS[name].families.items() if s == HOLDS}
    return got | ({"F"} if any(name in names for _, names in FIXED.values()) else set())


# ---- scenes -----------------------------------------------------------------------------------------------------------------

def inputs_of(gt, pred):
    """Every input role, [1,H,W] each, from a ground-truth and a predicted id map [H,W]."""
    gt, pred = np.asarray(gt).astype(np.int32), np.asarray(pred).astype(np.int32)
    H, W = gt.shape
    yy, xx = np.mgrid[0:H, 0:W]
    region = (gt > 0) | (pred > 0)
    seeds = np.where((gt > 0) & ((yy * 7 + xx * 3) % 5 == 0), gt, 0)
    under = np.where(region, 3 + (yy * 3 + xx * 5) % 11, 0)
    x = {"ids": gt, "ids2": pred, "mask": (gt > 0).astype(np.uint8), "mask2": (pred > 0).astype(np.uint8), "region": region.astype(np.uint8),
         "seeds": seeds, "image": ((yy // 2) * 3 + (xx // 3) * 5 + gt) % 7, "image16": (yy * 131 + xx * 71 + gt * 17) % 65536,
         "under": under, "marker": np.where(seeds > 0, under, 0)}
    return {k: np.ascontiguousarray(v[None]).astype(np.uint8 if v.dtype == np.uint8 else np.int32) for k, v in x.items()}


def composed_scene():
    """(gt, pred) int32 [41,45]: two touching cells (1, 2), a cell with a hole (3), two blobs joined by a one-pixel bridge (4), a
    pair in diagonal contact only (5, 6: one component when 8-connected, two when 4-connected), a one-pixel cell (7) and a disc
    (8); pred is the 4-connected labelling of the cells moved by (1, -1).  A background margin of 2 pixels at the least."""
    g = np.zeros((41, 45), np.int32)
    g[3:13, 4:11], g[3:13, 11:19] = 1, 2
    g[3:15, 23:35] = 3
    g[7:11, 27:31] = 0
    g[18:26, 4:10], g[18:26, 14:20], g[21, 10:14] = 4, 4, 4
    g[17:23, 25:30], g[23:29, 30:36] = 5, 6
    g[33, 8] = 7
    yy, xx = np.mgrid[0:41, 0:45]
    g[(yy - 32) ** 2 + (xx - 21) ** 2 <= 25] = 8
    import instances_ref
    moved = np.zeros_like(g)
    moved[1:, :-1] = g[:-1, 1:]
    return g, instances_ref.label(moved)[0]


def shape_scene(H, W):
    """Inputs of an H x W image of seeded cells (instances_ref.cells_case), both classes present whatever the size."""
    import instances_ref
    gt, pred = instances_ref.cells_case(H * W % 97, max(2, H * W // 150), H, W)
    gt[0, 0] = 0
    gt[-1, -1] = max(1, gt[-1, -1])
    return inputs_of(gt, pred)


def reused_scenes():
    """[(name, inputs)]: the generators the per-op tests already have, as scenes of families D and R."""
    import boundary_ref
    import instances_ref
    import rand_ref
    import shape_ref
    import track_ref
    label = lambda m: instances_ref.label(m)[0]
    busy = dict(shape_ref.size_cases(65, 66))["busy B2"]
    pair = boundary_ref.cells_pair()
    frames = track_ref.shifted_cells(3, 2, 48, 72, 9)
    ties = rand_ref.tie_maps(33, 31)
    pred, gt = rand_ref.speckle_pairs()
    return [("serpentine 67x129", inputs_of(3 * instances_ref.serpentine(67, 129), label(instances_ref.serpentine(129, 67).T))),
            ("busy 65x66", inputs_of(label(busy[0]), label(busy[1]))),
            ("cells 64x80", inputs_of(*instances_ref.cells_case(4, 12, 64, 80))),
            ("cells pair 64x80", inputs_of(label(pair[1]), 2 * label(pair[0]))),
            ("shifted cells 48x72", inputs_of(frames[1], frames[0])),
            ("ties 33x31", inputs_of(ties[5], ties[17])),
            ("speckle 70x90", inputs_of(gt[0], pred[0]))]


def strip_scene():
    """(gt, pred) int32 [3,40]: cells of a few widths along a strip with a background column left and right in both maps, touching pairs among them."""
    g = np.zeros((3, 40), np.int32)
    for k, (a, b) in enumerate(((1, 4), (4, 9), (11, 12), (14, 22), (22, 25), (27, 37)), start=1):
        g[k % 2:3, a:b] = k
    p = np.zeros_like(g)
    p[:, 2:] = g[:, :-2] > 0
    p[1, 8:10] = 0
    return g, p * 3


def margin(a):
    """The width of the background frame of a plane"""
    ys, xs = np.nonzero(np.asarray(a))
    H, W = np.shape(a)
    return min(ys.min(), xs.min(), H - 1 - ys.max(), W - 1 - xs.max()) if len(ys) else min(H, W)


def batch_of(x, two_class=False):
    """B = 3: an empty, a full and the ordinary image x ([1,H,W] each role); two_class leaves one pixel of the other class in
    the empty and in the full image (an op that refuses a one-class image)."""
    out = {}
    for k, a in x.items():
        empty, full = np.zeros_like(a[0]), np.full_like(a[0], 5 if a.dtype != np.uint8 else 1)
        if k in ("image", "image16", "under", "marker"):
            empty, full = a[0] % 3, a[0][::-1, ::-1] + 1
        elif two_class:
            empty[0, 0], full[-1, -1] = 1, 0
        out[k] = np.stack([empty, full, a[0]])
    return out


BATCH_ORDERS = ((0, 1, 2), (2, 0, 1), (1, 2, 0))


# ---- the placement plan of family T -----------------------------------------------------------------------------------------

CANVAS = (131, 197)          # three and four 64-tiles, five and seven 32-tiles, W below 256, neither side a multiple of anything
OFFSETS_Y = (0, 23, 31, 32, 33, 63, 64, 65, 90)
OFFSETS_X = (0, 19, 31, 32, 33, 63, 64, 65, 127, 152)
STRIP_CANVAS = (3, 300)
STRIP_X = (0, 215, 216, 217, 255, 256, 260)
PERIODS = (32, 64)           # LB_TILE of label.hip and the tiles of prepare.hip; the tiles of sweep.hpp / warp.hip / measure.hip, the
                             # 64 columns of a dm.hpp workgroup and the 64 lanes of a wave


def on_lattice(o, lattice):
    """The offset of the lattice next to o, on the far side of a seam of period 32 that o + 1 lies on (31 -> 30, 33 -> 34)."""
    if o % lattice == 0:
        return o
    return o - o % lattice if (o + 1) % 32 == 0 else o + lattice - o % lattice


def placements(h, w, canvas=CANVAS, ys=OFFSETS_Y, xs=OFFSETS_X, limit=48, lattice=1):
    """At most `limit` offsets (dy, dx) of an h x w scene in the canvas: every dy and every dx of the lists (the largest moved so
    that the scene ends in the last row / column), each dy with four dx, and the diagonal pairs where two seams cross.  lattice:
    for an op whose definition names absolute coordinates modulo the lattice, the offsets are moved onto it."""
    H, W = canvas
    assert (H - h) % lattice == 0 and (W - w) % lattice == 0
    ys = sorted({min(on_lattice(y, lattice), H - h) for y in ys} | {H - h})
    xs = sorted({min(on_lattice(x, lattice), W - w) for x in xs} | {W - w})
    plan = []
    for i, dy in enumerate(ys):
        for j in range(max(4, -(-len(xs) // len(ys)))):
            plan.append((dy, xs[(i + 3 * j) % len(xs)]))
    plan += [(d, d) for d in ys if d in xs]
    plan = list(dict.fromkeys(plan))
    return plan[:limit] if len(plan) > limit else plan


def seam_gaps(plan, h, w, canvas=CANVAS, periods=PERIODS, lattice=1):
    """The seam conditions a plan misses (empty: it meets them all): on each axis and for each period m a placement that starts
    at m - 1, at m and at m + 1 (m - lattice and m + lattice on a lattice) and one with a seam through the scene's interior; one
    that ends in the last row, one in the last column."""
    gaps = []
    for axis, size, end in ((0, h, canvas[0]), (1, w, canvas[1])):
        starts = {p[axis] for p in plan}
        for m in periods:
            gaps += ["axis %d: no start at %d" % (axis, s) for s in (m - lattice, m, m + lattice) if s not in starts]
            if not any(o < k * m < o + size - 1 for o in starts for k in range(1, end // m + 1)):
                gaps.append("axis %d: no seam of period %d inside the scene" % (axis, m))
        if end - size not in starts:
            gaps.append("axis %d: no placement ends at the canvas's end" % axis)
    return gaps


# ---- the relations ----------------------------------------------------------------------------------------------------------
# Each returns the number of comparisons it made and raises AssertionError at the first that fails.

def _all_ids(op, x):
    return np.unique(np.concatenate([x[k].ravel() for k in op.id_inputs]))


def _demand(name, family, what, a, b, include=None):
    """The two normal forms have the same fields and are equal bit for bit, but for the fields the table says family `family` of
    the op does not carry (Op.omits); include names one of those to compare all the same (what its counterexample does)."""
    assert set(a) == set(b), "%s, %s: fields %s / %s" % (name, what, sorted(a), sorted(b))
    drop = set(OPS[name].omits.get(family, ())) - {include}
    assert drop <= set(a), "%s: omitted fields %s are not in the normal form" % (name, sorted(drop - set(a)))
    bad = same({k: v for k, v in a.items() if k not in drop}, {k: v for k, v in b.items() if k not in drop})
    assert bad is None, "%s, %s: %r differs" % (name, what, bad)


def relation_D(name, x, backend, views=VIEWS[1:], include=None):
    """unview(op(view(x, v)), v) == op(x)"""
    base = run(name, x, backend)
    for v in views:
        tr = Tr(v=v, shape=view(x[OPS[name].inputs[0]], v).shape[-2:])
        _demand(name, "D", "view %d of %s" % (v, x[OPS[name].inputs[0]].shape[-2:]), run(name, tr.apply(x), backend, tr), base, include)
    return len(views)


def relation_T(name, x, backend, canvas, plan, include=None):
    """extract(op(embed(scene, dy, dx))) == extract(op(embed(scene, 0, 0)))"""
    h, w = x[OPS[name].inputs[0]].shape[-2:]
    at = lambda dy, dx: Tr(shape=canvas, shift=(dy, dx), scene=(h, w))
    base = run(name, at(0, 0).apply(x), backend, at(0, 0))
    plan = [p for p in plan if p != (0, 0)]
    for dy, dx in plan:
        _demand(name, "T", "scene at (%d, %d) of %s" % (dy, dx, canvas), run(name, at(dy, dx).apply(x), backend, at(dy, dx)), base, include)
    return len(plan)


def relation_B(name, x, backend, orders=BATCH_ORDERS):
    """op(stack)[b] == op(x_b) for an empty, a full and an ordinary image, in three orders"""
    three = batch_of(x, OPS[name].two_class)
    alone = [run(name, {k: a[b:b + 1] for k, a in three.items()}, backend) for b in range(3)]
    for order in orders:
        got = run(name, {k: a[list(order)] for k, a in three.items()}, backend)
        for at, b in enumerate(order):
            _demand(name, "B", "image %d at place %d of the batch %s" % (b, at, order), pick(got, at), pick(alone[b], 0))
        for k, v in got.items():                              # the integer words of a whole batch: the sum over its images
            if k.startswith("batch:") and np.asarray(v).dtype.kind == "i":
                assert np.array_equal(v, sum(a[k] for a in alone)), "%s, batch %s: %r is not the sum over the images" % (name, order, k)
    return 3 * len(orders)


def relation_R(name, x, backend, f, include=None):
    """op(f(ids)) == f(op(ids)): per-id outputs permuted, scores identical"""
    op = OPS[name]
    tr = Tr(f=f, ids=_all_ids(op, x))
    _demand(name, "R", "ids renamed", run(name, tr.apply(x, op.id_inputs), backend, tr), run(name, x, backend), include)
    return 1


def renamings(name, x):
    """The renamings family R uses for an op: order preserving (3 i + 5, and up to 2^24 - 1 where no table is sized by the
    largest id) for the ops whose ties go to the smaller id, permutations onto ids with gaps for the others."""
    op = OPS[name]
    ids = _all_ids(op, x)
    if op.relabel == "order":
        return [order_map] + ([] if name == "link_frames" else [top_map(int(ids.max()))])
    return [gap_permutation(ids[ids > 0], seed) for seed in (0, 1)]
