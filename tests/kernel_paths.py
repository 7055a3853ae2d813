"""Which kernels an op actually reached: a recorder over the library's per-launch profile (unet_profile_*).

    with kernel_paths.record() as rec:
        L.unet_conv3x3_fwd(...)
    assert "igemmb3<0>" in rec.families

Every launch site brackets its kernel with a tagged record (`igemmb3<1> M=... N=...`, `wgrad<2;2;2;split3> buf=0 Ci=...`,
`wino32<0> ...`); a kernel *family* is the tag up to its first space, so it names the kernel and its template arguments
(tile shape, padding, staging variant) and nothing about the shape of the call.  The dispatch predicates of the library
(wino_applicable, igemmb3_applicable, convb64_applicable, up_applicable, wgradw_applicable, the Nn % 128 tile choice,
the nP >= 64 reduce width) decide the family; the tests pin each case to the family it is meant to exercise, so a
change to a predicate that moves coverage elsewhere fails loudly instead of silently.

A plain helper module (imported like weighted_map_ref), not a conftest."""
import contextlib
import csv
import os
import tempfile


class Record:
    def __init__(self):
        self.rows = []            # dicts: kind, ms, gflop, exec_gflop, mbytes, row, tag

    @property
    def tags(self):
        return [r["tag"] for r in self.rows]

    @property
    def families(self):
        """Kernel families in launch order (duplicates kept)."""
        return [family(t) for t in self.tags]

    def family_set(self):
        return set(self.families)

    def fields(self, fam):
        """key=value fields of the launches of one family (e.g. buf, pad, groups)."""
        out = []
        for t in self.tags:
            if family(t) == fam:
                out.append(dict(kv.split("=", 1) for kv in t.split(" ")[1:] if "=" in kv))
        return out

    def reached(self, spec):
        """spec = a family, optionally followed by key=value fields that one launch of it must carry
        (e.g. "wgrad<3;3;1;split3> buf=0")."""
        fam, *kvs = spec.split(" ")
        want = dict(kv.split("=", 1) for kv in kvs)
        return any(all(f.get(k) == v for k, v in want.items()) for f in self.fields(fam))

    def main_families(self, reduces=True):
        """Families of the contraction launches (implicit GEMM, Winograd, weight gradient and, unless reduces=False, its
        split-K reduce) in launch order."""
        kinds = (K_IGEMM, K_WINO, K_WGRAD, K_REDUCE) if reduces else (K_IGEMM, K_WINO, K_WGRAD)
        return [family(r["tag"]) for r in self.rows if r["kind"] in kinds]

    def __repr__(self):
        return "Record(%s)" % ", ".join(self.families)


def family(tag):
    return tag.split(" ", 1)[0]


def parse(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    for r in rows:
        r["kind"] = int(r["kind"])
    return rows


@contextlib.contextmanager
def record(lib=None):
    """Reset and enable the profile with every launch kind selected, run the body, synchronise, dump and parse.  Profiling
    is always switched off again on exit, also when the body raises.  Not re-entrant: a nested record() empties the outer one."""
    import torch
    if lib is None:
        import _hip
        lib = _hip.lib()
    rec = Record()
    _ok(lib.unet_profile_reset(), "unet_profile_reset")
    _ok(lib.unet_profile_select(0xFFFFFFFF), "unet_profile_select")
    _ok(lib.unet_profile_enable(1), "unet_profile_enable")
    try:
        yield rec
        torch.cuda.synchronize()
        fd, path = tempfile.mkstemp(suffix=".csv", prefix="unet_paths_")
        os.close(fd)
        try:
            _ok(lib.unet_profile_dump(path.encode()), "unet_profile_dump")
            rec.rows = parse(path)
        finally:
            os.remove(path)
    finally:
        lib.unet_profile_enable(0)
        lib.unet_profile_reset()


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (what, rc))


def cdiv(a, b):
    return -(-a // b)


# ---- the one size rule (csrc/common.hpp) ------------------------------------------------------------------------------------
LIMIT_31BIT = 0x7FFFFFFF


def tensor_bytes(B, H, W, C, es=4):
    return B * H * W * C * es


def fits_buffer(nbytes):
    """common.hpp fits_buffer: a tensor is staged through a buffer descriptor only while its bytes stay below 2^31 - 1."""
    return nbytes < LIMIT_31BIT


def staging(dma, nbytes=()):
    """The effective staging variant of an MFMA launch (the <1> / <0> of wino32 and wgradw, the buf= field of igemm and wgrad):
    the unet_set_lds_dma knob AND every tensor the launch stages fitting a buffer descriptor.  nbytes: the bytes of those
    tensors (the sources of a forward or dgrad, x and dz of a weight gradient); empty = all small, the knob alone decides."""
    return int(bool(dma) and all(fits_buffer(b) for b in nbytes))


def wino_applicable(OW, Nn, nchs, OH=None):
    """wino.hip wino_applicable for the per-op shapes (square tiles, linear store)."""
    OH = OW if OH is None else OH
    return Nn % 32 == 0 and cdiv(OW, 2) >= 9 and cdiv(OH, 2) >= 7 and all(c % 8 == 0 for c in nchs)


def fp32_conv_family(mode, dma, OW, Nn, nchs, pad=False, nbytes=()):
    """The family an fp32-mode (0 / 3) single 3x3 launch reaches: Winograd (staging variant = the lds_dma knob AND the sources'
    bytes, staging()) in mode 3 where wino_applicable holds, else the implicit GEMM tile chosen by Nn % 128 (its staging
    variant is the tag's buf= field: conv_spec)."""
    if mode == 3 and wino_applicable(OW, Nn, nchs):
        return "wino32<%d>" % staging(dma, nbytes)
    return "igemm<%s;%d>" % ("128;128" if Nn % 128 == 0 else "256;64", int(pad))


def bf16_conv_family(OW, Nn, nchs, pad):
    """The family a bf16-tensor (mode 2) 3x3 launch reaches (igemmb.hip launch_igemmb): the persistent 64-channel kernel for
    one 64-channel source, the band kernel for >= 19 outputs per row and whole 128-row tiles, else the implicit GEMM tile
    chosen by Nn % 128."""
    if len(nchs) == 1 and nchs[0] == 64 and Nn % 64 == 0:
        return "convb64<8;32>"
    if Nn % 128 == 0 and OW >= 19 and all(c % 64 == 0 for c in nchs):
        return "igemmb3<%d>" % int(pad)
    return "igemmb<%s;%d>" % ("128;128" if Nn % 128 == 0 else "256;64", int(pad))


def conv_family(mode, dma, OW, Nn, nchs, pad, nbytes=()):
    """The family of one 3x3 launch in any mode: fp32 (0 / 3), bf16x3 (1) or bf16 tensors (2)."""
    if mode == 2:
        return bf16_conv_family(OW, Nn, nchs, pad)
    if mode == 1:
        return "igemmx<%s;%d;split3>" % ("128;128" if Nn % 128 == 0 else "256;64", int(pad))
    return fp32_conv_family(mode, dma, OW, Nn, nchs, pad, nbytes)


def conv_spec(mode, dma, OW, Nn, nchs, pad=False, nbytes=()):
    """conv_family as a spec for Record.reached: an fp32 implicit GEMM also carries its staging variant (buf=)."""
    fam = conv_family(mode, dma, OW, Nn, nchs, pad, nbytes)
    return fam + " buf=%d" % staging(dma, nbytes) if fam.startswith("igemm<") else fam


def taps_leave(src_H, OH, o0, src_pad):
    """launch_igemm's "padded" test for a 3x3 launch over output rows [o0, o0 + OH) of a source of src_H rows zero-padded by
    src_pad: some tap falls outside the source (square tiles, so rows decide)."""
    return o0 - src_pad < 0 or OH - 1 + o0 - src_pad + 2 >= src_H


def concat_fwd_families(mode, dma, Hs, pad, C1, C2, K, split_thr=0.85):
    """The launches of unet_conv3x3_fwd over the virtual concat (net.hip conv_fwd_launch): one two-source launch, or - a
    zero-padded skip source in the fp32 modes, when its window is small enough - the up-conv source over the full domain
    followed by the skip source over its window (accumulating in place)."""
    H = Hs + 2 * pad
    Ho = H - 2
    w0, w1 = max(pad - 2, 0), min(pad + Hs, Ho)
    if not (pad > 0 and mode != 2 and (w1 - w0) ** 2 < split_thr * Ho * Ho):
        return [conv_family(mode, dma, Ho, K, [C1, C2], taps_leave(Hs, Ho, 0, pad))]
    return [conv_family(mode, dma, Ho, K, [C2], False),
            conv_family(mode, dma, w1 - w0, K, [C1], taps_leave(Hs, w1 - w0, w0, pad))]


def wgrad_family(mode, dma, Ci, Cj, nbytes=()):
    """The 3x3 weight-gradient kernel of a source with Ci channels against dz with Cj channels (nbytes: the bytes of both)."""
    if mode == 2:
        return "wgradb<3;3;1>"
    if mode == 1:
        return "wgrad<3;3;1;split3>"
    if mode == 3 and Ci % 64 == 0 and Cj % 64 == 0:
        return "wgradw<%d>" % staging(dma, nbytes)
    return "wgrad<3;3;1;split0>"


def wgrad_spec(mode, dma, Ci, Cj, nbytes=()):
    """wgrad_family as a spec for Record.reached: the row-walking kernels carry their staging variant as buf= (the exact fp32
    3x3 instantiation has the global_load_lds form only, wgrad.hip CAN_BUF; the bf16 one the buffer form only)."""
    fam = wgrad_family(mode, dma, Ci, Cj, nbytes)
    if fam == "wgrad<3;3;1;split0>":
        return fam + " buf=0"
    if fam == "wgrad<3;3;1;split3>":
        return fam + " buf=%d" % staging(dma, nbytes)
    return fam + (" buf=1" if mode == 2 else "")


def upconv_wgrad_spec(mode, dma, nbytes=()):
    """The up-conv weight gradient (wgrad.hip up_applicable): the pixel-linear kernel for bf16 tensors and, while both tensors
    fit a buffer descriptor and the knob is on, for exact fp32; else the row-walking 2x2 stride-2 kernel."""
    if mode == 2:
        return "wgrad_up<bf16>"
    if mode != 1 and staging(dma, nbytes):
        return "wgrad_up<f32>"
    return "wgrad<2;2;2;split%d> buf=%d" % (3 if mode == 1 else 0, staging(dma, nbytes))


def concat_bwd_families(mode, dma, Hs, pad, C1, C2, K):
    """The contraction launches of unet_conv3x3_bwd over the virtual concat with every output requested, reduces left out:
    dgrad of source 1 (the crop of the padded region), dgrad of source 2, then each source's weight gradient."""
    H = Hs + 2 * pad
    Ho = H - 2
    return [conv_family(mode, dma, Hs, C1, [K], taps_leave(Ho, Hs, pad, 2)), conv_family(mode, dma, H, C2, [K], True),
            wgrad_family(mode, dma, C1, K), wgrad_family(mode, dma, C2, K)]


def single_pad_fwd_family(mode, dma, Hs, pad, C1, K):
    """The one launch of unet_conv3x3_fwd over a single source of extent Hs with a signed pad (x2 = NULL, H = Hs + 2 pad):
    a positive pad makes taps leave the source, a negative one crops it and none does."""
    Ho = Hs + 2 * pad - 2
    return conv_family(mode, dma, Ho, K, [C1], taps_leave(Hs, Ho, 0, pad))


def single_pad_bwd_families(mode, dma, Hs, pad, C1, K):
    """The contraction launches of unet_conv3x3_bwd over that single padded source with every output requested, reduces left
    out: the dgrad over the source's window of the virtual input, then its weight gradient (the bias gradient does not ride
    on a launch that misses part of dz: it is the stand-alone bias_grad)."""
    Ho = Hs + 2 * pad - 2
    return [conv_family(mode, dma, Hs, C1, [K], taps_leave(Ho, Hs, pad, 2)), wgrad_family(mode, dma, C1, K)]


# kernel kinds of the profile (include/unet_hip.h, "measurement")
K_IGEMM, K_WGRAD, K_REDUCE, K_WINO, K_CONV11C, K_ELEMWISE = 0, 1, 2, 3, 4, 5
