// net.hip — the C ABI of libunet_hip.so: plan, workspace layout, Unet forward / backward
// orchestration and the per-op entry points (see include/unet_hip.h for the contract and the
// reference lines each entry point replaces).
#include "common.hpp"
#include "plans.hpp"
#include "../../include/unet_hip.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace unet {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static float *g_zero[64] = {nullptr};
static std::mutex g_zero_mu;
const float *zero_page()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { set_error("zero_page: bad device"); return nullptr; }
    std::lock_guard<std::mutex> lk(g_zero_mu);
    if (!g_zero[dev]) {
        float *p = nullptr;
        if (hipMalloc((void **)&p, 4096) != hipSuccess || hipMemset(p, 0, 4096) != hipSuccess) {
            set_error("zero_page: hipMalloc failed");
            return nullptr;
        }
        g_zero[dev] = p;
    }
    return g_zero[dev];
}

// ---- the network, stated once ---------------------------------------------------------------------
// Everything that depends on the shape of the network (parameter sizes, workspace plan, profile rows, flop counts, forward
// and backward walks, backward stages) reads this table.
enum { K_CONV1, K_CONV, K_CAT, K_UP, K_HEAD };          // conv11c (1 input channel) / 3x3 conv / 3x3 conv over the virtual concat / up-conv / head
enum { T_A1, T_A2, T_T, T_U, T_D1, T_D2, N_TENSORS, T_NONE = N_TENSORS };   // activation tensors of a level (TENSOR_NAME)
struct Layer {
    const char *name;     // LAYER_NAME: profile rows are "<name>.<fwd|dgrad|wgrad|bwd>" (bench.py maps them onto SURVEY 8a rows)
    int kind, level;
    int ci, co;           // the levels whose width (base_ch << level) the input / output channels are; -1: 1 channel in, n_classes out
    int stage;            // backward stage (reverse layer order, so gradient buckets complete early for the all-reduce)
    int in, out;          // tensor read (at level ci; K_CAT: the padded skip t[level] next to u[level]) and written (at level)
    int drop = -1;        // drop-out site of the layer's output (Ronneberger et al. 2015, section 3.1; dropout.hip), -1: none
};
// the reference's declaration order (network.py:23-58) = forward order; the backward walks each stage's layers in reverse
static const Layer LAYERS[UNET_N_LAYERS] = {
    {"conv11c", K_CONV1, 0, -1, 0, 5, T_NONE, T_A1}, {"conv12c", K_CONV, 0, 0, 0, 5, T_A1, T_A2},
    {"conv21c", K_CONV, 1, 0, 1, 5, T_T, T_A1},      {"conv22c", K_CONV, 1, 1, 1, 5, T_A1, T_A2},
    {"conv31c", K_CONV, 2, 1, 2, 5, T_T, T_A1},      {"conv32c", K_CONV, 2, 2, 2, 5, T_A1, T_A2},
    {"conv41c", K_CONV, 3, 2, 3, 5, T_T, T_A1},      {"conv42c", K_CONV, 3, 3, 3, 5, T_A1, T_A2, 0},
    {"conv51c", K_CONV, 4, 3, 4, 4, T_T, T_A1},      {"conv52c", K_CONV, 4, 4, 4, 4, T_A1, T_A2, 1},
    {"upconv4", K_UP, 3, 4, 3, 3, T_A2, T_U}, {"conv41e", K_CAT, 3, 4, 3, 3, T_T, T_D1}, {"conv42e", K_CONV, 3, 3, 3, 3, T_D1, T_D2},
    {"upconv3", K_UP, 2, 3, 2, 2, T_D2, T_U}, {"conv31e", K_CAT, 2, 3, 2, 2, T_T, T_D1}, {"conv32e", K_CONV, 2, 2, 2, 2, T_D1, T_D2},
    {"upconv2", K_UP, 1, 2, 1, 1, T_D2, T_U}, {"conv21e", K_CAT, 1, 2, 1, 1, T_T, T_D1}, {"conv22e", K_CONV, 1, 1, 1, 1, T_D1, T_D2},
    {"upconv1", K_UP, 0, 1, 0, 0, T_D2, T_U}, {"conv11e", K_CAT, 0, 1, 0, 0, T_T, T_D1}, {"conv12e", K_CONV, 0, 0, 0, 0, T_D1, T_D2},
    {"finalconv", K_HEAD, 0, 0, -1, 0, T_D2, T_NONE}};
enum { C11C = 0, FINAL = UNET_N_LAYERS - 1 };
static const int N_STAGES = 6;
// unet_debug_buffer's names: "<tensor>_<level>", "g_<tensor>_<level>" for the gradient
static const struct { const char *name; int levels; } TENSOR_NAME[N_TENSORS] = {{"a1", 5}, {"a2", 5}, {"t", 4}, {"u", 4}, {"d1", 4}, {"d2", 4}};

// one activation tensor, NHWC [B, e, e, c]: workspace offset of the tensor and (training) of its gradient
struct Act { size_t off = 0, g = 0; int e = 0, c = 0; };

struct Plan {
    int B = 0, S = 0, base = 0, So = 0, training = 0;
    int ncls = 2;         // classes of the head (finalconv's output channels)
    int math = 3;         // arithmetic, fixed when the forward is planned: the backward of that forward uses the same
    float drop_p = 0.f;   // unet_forward_dropout: drop probability of this forward (0: none); the backward scales by 1 / (1 - p)
    unsigned long long drop_seed = 0, drop_step = 0;
    bool drops(const Layer &L) const { return L.drop >= 0 && drop_p > 0.f; }
    int ch[5], pad[4];    // pad > 0: the skip t[l] is zero-padded to u[l]'s extent, pad < 0: cropped
    // per level: the two encoder convs' outputs, the pool's, the up-conv's, the two decoder convs'
    Act a1[5], a2[5], t[4], u[4], d1[4], d2[4];
    size_t g_ts[4];       // the skip half of conv_l1e's dgrad; added to g_t by the dgrad of the conv that reads t[l]
    size_t wt_fwd[UNET_N_LAYERS], wt_bwd[UNET_N_LAYERS];
    size_t wu_fwd[UNET_N_LAYERS], wu_bwd[UNET_N_LAYERS];     // Winograd-transformed filters (math mode 3), 16/9 of the 3x3 layers
    size_t slab = 0, slab_bytes = 0, small = 0, small_bytes = 0, xin = 0;
    size_t total = 0;
    const Act &act(int tensor, int l) const { const Act *const v[N_TENSORS] = {a1, a2, t, u, d1, d2}; return v[tensor][l]; }
    const Act &in(const Layer &L) const { return act(L.in, L.kind == K_CAT ? L.level : L.ci); }     // K_CAT: the skip; u[level] is the other
    const Act &out(const Layer &L) const { return act(L.out, L.level); }
};

}  // namespace unet

using namespace unet;

struct unet_dp;       // dp.hip: RCCL communicator + its stream (null until unet_dp_init)
int unet_dp_free(unet_dp *d);

struct unet_handle {
    int base_ch;
    int device;
    int math;             // arithmetic of this handle's forwards (unet_config::math); -1 = the process default at each forward
    int n_classes = 2;    // unet_create_classes: output channels of the head, 2..UNET_MAX_CLASSES
    unet_dp *dp = nullptr;
    float grad_scale = 1.f;   // unet_set_grad_scale: the backward reads dlogits * grad_scale (data parallel: 1/world)
    // opt-in (unet_set_overlap / UNET_OVERLAP=1): the weight gradients of a backward stage run on an auxiliary stream next to
    // the dgrad chain (they only share dz); the streams re-join at the end of every stage
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // plans of this handle's training forwards, keyed by workspace pointer: pending until their last backward stage has been
    // enqueued, then finished and evicted oldest first (plans.hpp has the contract)
    PlanRegistry<Plan> live;
};

unet_dp **unet_handle_dp_slot(unet_handle *h) { return &h->dp; }
int unet_handle_device(const unet_handle *h) { return h->device; }

namespace unet {

// Arithmetic mode of the C-ABI call this thread is in; the descriptor builders copy it into every launch descriptor
// (handle entry points: the plan's mode; per-op entry points: the process default).
static thread_local int t_math = 3;
static thread_local int t_es = 4;            // element size of activations / activation gradients / packed filters: 2 (bf16) in mode 2
struct MathScope {
    int prev;
    explicit MathScope(int m) : prev(t_math) { t_math = m; t_es = m == 2 ? 2 : 4; }
    ~MathScope() { t_math = prev; t_es = prev == 2 ? 2 : 4; }
};
// pointer arithmetic on tensors whose element size depends on the mode (the descriptors carry them as float*)
static inline float *adv(float *p, size_t elems) { return (float *)((char *)p + elems * t_es); }


static int layer_ci(int base, const Layer &L) { return L.ci < 0 ? 1 : base << L.ci; }
static int layer_co(int base, const Layer &L, int ncls) { return L.co < 0 ? ncls : base << L.co; }
static int layer_taps(const Layer &L) { return L.kind == K_UP ? 2 : L.kind == K_HEAD ? 1 : 3; }       // k of its k x k filter

static size_t layer_numel(int base, int layer, bool bias, int ncls = 2)
{
    const Layer &L = LAYERS[layer];
    const int k = layer_taps(L);
    return bias ? (size_t)layer_co(base, L, ncls) : (size_t)layer_ci(base, L) * layer_co(base, L, ncls) * k * k;
}

// floats of the Winograd U matrix of a layer (0 for the layers wino.hip does not serve: conv11c, up-convs, head)
static size_t layer_wino_floats(int base, int layer)
{
    const Layer &L = LAYERS[layer];
    if (L.kind != K_CONV && L.kind != K_CAT) return 0;
    // U is kept in whole 64-row blocks (wino_u_floats); forward: rows = output channels, one sub-matrix per source of the
    // virtual concat; dgrad: rows = input channels, one launch (and sub-matrix) per source.  The larger of the two directions.
    const int ci = layer_ci(base, L), co = layer_co(base, L, 2);
    const size_t fwd = wino_u_floats(ci, co);
    const size_t bwd = L.kind == K_CAT ? 2 * wino_u_floats(co, ci / 2) : wino_u_floats(co, ci);
    return fwd > bwd ? fwd : bwd;
}

// One 3x3 layer's reference (OIHW) weights and their packed igemm copy.  The copy is made on first need: in math mode 3
// most launches take the Winograd path, whose filter transform reads the reference weights directly.
struct WLayer {
    const float *w; int O, I;      // reference tensor [O][I][3][3]
    bool dgrad;                    // packed copy: forward [O][9*(C1|C2)] or dgrad [I][9*O]
    float *wt; int C1, C2;
    bool packed = false;
    int ensure_packed(hipStream_t st)
    {
        if (packed) return 0;
        packed = true;
        return dgrad ? pack_conv_dgrad(w, wt, O, I, t_es, st) : pack_conv_fwd(w, wt, O, C1, C2, t_es, st);
    }
};

// Route a 3x3 launch: math mode 3 and a shape wino.hip takes -> transform the filters (rows n0.., columns k0.. of the
// launch's filter matrix within the layer) into `wu`; otherwise make sure the packed igemm weights exist.
static int with_wino(IgemmP &p, float *wu, WLayer &L, int n0, int k0, hipStream_t st)
{
    if (p.math != 3 || !wu || !wino_applicable(p)) return L.ensure_packed(st);
    int kc = 0;
    for (int i = 0; i < p.nsrc; ++i) kc += p.src[i].nch;
    int rc = wino_transform_ref(L.w, L.I, L.dgrad ? 1 : 0, n0, p.Nn, k0, kc, wu, st);
    if (rc) return rc;
    p.wino_u = wu;
    return 0;
}

static int check_size(int S)
{
    if (S < 60 + 16 * 8 || (S - 60) % 16 != 0 || ((S - 60) / 16) % 2 != 0) {
        set_error("input size %d is not 16L+60 with L even >= 8: the reference's crop_and_concat/torch.cat "
                  "raises on it (network.py:124-127)", S);
        return UNET_E_BADSIZE;
    }
    return 0;
}

// profile row of a launch group: "<layer>.<fwd|dgrad|wgrad>"
struct RowScope : ProfScope {
    static const char *make(char (&buf)[40], int layer, const char *what) { snprintf(buf, sizeof(buf), "%s.%s", LAYERS[layer].name, what); return buf; }
    char buf[40];
    RowScope(int layer, const char *what) : ProfScope(make(buf, layer, what)) {}
};

// ---- descriptor builders (shared by the plan sizing and the launches) ----------------------------
static IgemmP conv_fwd_desc(const float *x1, int H1, int W1, int C1, int pad1, const float *x2, int C2,
                            int B, int H, int W, const float *wt, const float *bias, int K, int relu, float *y)
{
    IgemmP p{};
    p.nsrc = x2 ? 2 : 1;
    p.src[0] = GSrc{x1, H1, W1, C1, 0, C1, pad1};
    if (x2) p.src[1] = GSrc{x2, H, W, C2, 0, C2, 0};
    p.wt = wt; p.Kd = 9 * (C1 + C2);
    p.T = 9; p.TX = 3; p.stride = 1; p.oy0 = 0; p.ox0 = 0;
    p.NB = B; p.OH = H - 2; p.OW = W - 2; p.M = B * p.OH * p.OW; p.Nn = K;
    p.dst = y; p.DH = p.OH; p.DW = p.OW; p.DC = K; p.dn0 = 0;
    p.bias = bias; p.relu = relu;
    p.math = t_math;
    return p;
}

// Forward 3x3 conv, over one source or over the virtual concat.  One launch: lazy pack or Winograd transform of the filters,
// and with `pool_dst` the 2x2 max-pool of the output written by the Winograd epilogue where that fuses (*pool_fused).
// When the skip source is zero-padded (pad > 0) its taps only
// reach the output window [pad-2, pad+H1): running it as part of one GEMM would spend 30-50 % of that
// layer's MFMA work on zeros.  So: launch 1 = up-conv source over the full domain (+bias, ReLU outside the
// window), launch 2 = skip source over the window only, accumulating in place (+ReLU).  Same math, same
// K order per source; the two partial sums are added in fp32.
static int conv_fwd_launch(const float *x1, int H1, int C1, int pad1, const float *x2, int C2, int B, int H,
                           const float *w_oihw, float *wt, const float *bias, int K, int relu, float *y, hipStream_t st, float *wu = nullptr,
                           float *pool_dst = nullptr, bool *pool_fused = nullptr)
{
    const int Ho = H - 2;
    if (!x2) C2 = 0;
    WLayer L{w_oihw, K, C1 + C2, false, wt, C1, C2};
    int rc;
    int w0 = pad1 - 2; if (w0 < 0) w0 = 0;
    int w1 = pad1 + H1; if (w1 > Ho) w1 = Ho;
    static const double split_thr = [] { const char *e = getenv("UNET_SPLIT_THR"); return e ? atof(e) : 0.85; }();
    // (not with bf16 tensors: the partial sum between the two launches would be rounded to bf16 — a second rounding of
    //  the layer's output — and the zero-padded taps cost that mode no memory traffic, only cheap MFMA time)
    const bool split = x2 && pad1 > 0 && t_math != 2 && (double)(w1 - w0) * (w1 - w0) < split_thr * (double)Ho * Ho;
    if (!split) {
        IgemmP p = conv_fwd_desc(x1, H1, H1, C1, pad1, x2, C2, B, H, H, wt, bias, K, relu, y);
        if ((rc = with_wino(p, wu, L, 0, 0, st))) return rc;
        if (pool_dst && p.wino_u && wino_fuses_pool(p)) { p.pool_dst = pool_dst; *pool_fused = true; }
        return launch_igemm(p, st);
    }
    const int ldw = 9 * (C1 + C2);
    IgemmP a = conv_fwd_desc(x2, H, H, C2, 0, nullptr, 0, B, H, H, adv(wt, 9 * C1), bias, K, relu, y);
    a.ldw = ldw;
    if (relu) { a.rw0 = w0; a.rw1 = w1; }
    if ((rc = with_wino(a, wu, L, 0, C1, st))) return rc;
    if ((rc = launch_igemm(a, st))) return rc;
    IgemmP b = conv_fwd_desc(x1, H1, H1, C1, pad1, nullptr, 0, B, H, H, wt, nullptr, K, relu, y);
    b.ldw = ldw;
    b.OH = b.OW = w1 - w0; b.M = B * b.OH * b.OW; b.oy0 = b.ox0 = w0;
    b.scatter = 2; b.dwy0 = b.dwx0 = w0; b.DH = b.DW = Ho;
    b.add = y;
    if ((rc = with_wino(b, wu ? wu + wino_u_floats(C2, K) : nullptr, L, 0, 0, st))) return rc;
    return launch_igemm(b, st);
}

// 2x2 stride-2 transposed conv as a GEMM over the input pixels: [B*H*W, Ci] x [Ci, 4*Co], scattered to [B, 2H, 2W, Co]
static IgemmP upconv_fwd_desc(const float *x, int B, int H, int W, int Ci, const float *wt, const float *bias, int Co, float *y)
{
    IgemmP u{};
    u.nsrc = 1; u.src[0] = GSrc{x, H, W, Ci, 0, Ci, 0};
    u.wt = wt; u.Kd = Ci;
    u.T = 1; u.TX = 1; u.stride = 1;
    u.NB = B; u.OH = H; u.OW = W; u.M = B * H * W; u.Nn = 4 * Co;
    u.dst = y; u.DH = 2 * H; u.DW = 2 * W; u.DC = Co; u.scatter = 1; u.cout = Co;
    u.bias = bias;
    u.math = t_math;
    return u;
}

// its dgrad: a 2x2 stride-2 conv of dy [B, 2H, 2W, Co], masked by the ReLU output the up-conv read
static IgemmP upconv_dgrad_desc(const float *dy, int B, int H, int W, int Ci, const float *wt, int Co, float *dx, const float *mask)
{
    IgemmP d{};
    d.nsrc = 1; d.src[0] = GSrc{dy, 2 * H, 2 * W, Co, 0, Co, 0};
    d.wt = wt; d.Kd = 4 * Co;
    d.T = 4; d.TX = 2; d.stride = 2;
    d.NB = B; d.OH = H; d.OW = W; d.M = B * H * W; d.Nn = Ci;
    d.dst = dx; d.DH = H; d.DW = W; d.DC = Ci;
    d.mask = mask;
    d.math = t_math;
    return d;
}

// dgrad of a 3x3 valid conv: dx over the window [oy0, oy0+OHW) of the conv's (virtual) input
static IgemmP conv_dgrad_desc(const float *dz, int Ho, int Wo, int K, int B, int OHW, int o0,
                              const float *wt_rows, int Nn, float *dx, const float *mask, const float *add)
{
    IgemmP p{};
    p.nsrc = 1;
    p.src[0] = GSrc{dz, Ho, Wo, K, 0, K, 2};
    p.wt = wt_rows; p.Kd = 9 * K;
    p.T = 9; p.TX = 3; p.stride = 1; p.oy0 = o0; p.ox0 = o0;
    p.NB = B; p.OH = OHW; p.OW = OHW; p.M = B * OHW * OHW; p.Nn = Nn;
    p.dst = dx; p.DH = OHW; p.DW = OHW; p.DC = Nn; p.dn0 = 0;
    p.mask = mask; p.add = add;
    p.math = t_math;
    return p;
}

static WgradP conv_wgrad_desc(const float *X, int XH, int XC, int xpad, const float *dz, int Ho, int K, int B,
                              float *dw, int Ctot, int c_off, float *slab, size_t slab_bytes, float *db = nullptr)
{
    WgradP p{};
    p.X = X; p.XH = XH; p.XW = XH; p.XC = XC; p.xc0 = 0; p.xpad = xpad;
    p.Y = dz; p.YH = Ho; p.YW = Ho; p.YC = K; p.yc0 = 0;
    p.NB = B; p.stride = 1; p.TY = 3; p.TX = 3; p.oy0 = 0; p.ox0 = 0;
    int w0 = xpad - 2; if (w0 < 0) w0 = 0;
    int w1 = xpad + XH; if (w1 > Ho) w1 = Ho;
    p.ywin0 = w0; p.ywin1 = w1; p.xwin0 = w0; p.xwin1 = w1;
    p.Ci = XC; p.Cj = K;
    p.out = dw ? dw + (size_t)c_off * 9 : nullptr; p.si = 9; p.sj = (long)Ctot * 9; p.st = 1;
    p.slab = slab; p.slab_bytes = slab_bytes; p.db = db;
    p.math = t_math;
    return p;
}

static WgradP upconv_wgrad_desc(const float *x, int H, int Ci, const float *dy, int Co, int B, float *dw,
                                float *slab, size_t slab_bytes, float *db = nullptr)
{
    WgradP p{};
    p.X = dy; p.XH = 2 * H; p.XW = 2 * H; p.XC = Co; p.xc0 = 0; p.xpad = 0;
    p.Y = x; p.YH = H; p.YW = H; p.YC = Ci; p.yc0 = 0;
    p.NB = B; p.stride = 2; p.TY = 2; p.TX = 2; p.oy0 = 0; p.ox0 = 0;
    p.ywin0 = 0; p.ywin1 = H; p.xwin0 = 0; p.xwin1 = H;
    p.Ci = Co; p.Cj = Ci;
    p.out = dw; p.si = 4; p.sj = (long)Co * 4; p.st = 1;
    p.slab = slab; p.slab_bytes = slab_bytes;
    p.db = db; p.db_on_x = db ? 1 : 0;        // db[co] = sum dOut: X is dOut here
    p.math = t_math;
    return p;
}

// dgrad launches of a 3x3 conv, one per source that wants its gradient: the first source (C1 channels, extent H1, only its
// window at pad1 of the virtual input) and, over the virtual concat, the second (C2 channels, the full extent H; else C2 = 0)
static int conv_dgrad_launch(const float *dz, int Ho, int K, int B, const float *w_oihw, float *wt, float *wu, int H1, int C1, int pad1,
                             float *dx1, const float *mask1, const float *add1, int H, int C2, float *dx2, const float *mask2, hipStream_t st)
{
    WLayer L{w_oihw, K, C1 + C2, true, wt, 0, 0};
    int rc;
    if (dx1) {
        IgemmP d = conv_dgrad_desc(dz, Ho, Ho, K, B, H1, pad1, L.wt, C1, dx1, mask1, add1);
        if ((rc = with_wino(d, wu, L, 0, 0, st))) return rc;
        if ((rc = launch_igemm(d, st))) return rc;
    }
    if (dx2) {
        IgemmP d = conv_dgrad_desc(dz, Ho, Ho, K, B, H, 0, adv(L.wt, (size_t)C1 * 9 * K), C2, dx2, mask2, nullptr);
        if ((rc = with_wino(d, wu + wino_u_floats(K, C1), L, C1, 0, st))) return rc;
        if ((rc = launch_igemm(d, st))) return rc;
    }
    return 0;
}

// Stream of the weight-gradient launches of a backward stage: the caller's stream, or (overlap on) the handle's auxiliary
// stream after it has been made to wait for everything enqueued on the caller's stream so far - so a weight gradient must
// be enqueued BEFORE the dgrad it is to run next to.
struct WgradStream {
    unet_handle *h; hipStream_t main; bool overlap; bool used;
    hipError_t err = hipSuccess;     // sticky: a failed fork / join means the two streams are not ordered - the stage must not report success
    hipStream_t get()
    {
        if (!overlap) return main;
        // fork failed: the weight gradient stays on the caller's stream (ordered by construction)
        hipError_t e = hipEventRecord(h->ev_fork, main);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->aux, h->ev_fork, 0);
        if (e != hipSuccess) { if (err == hipSuccess) err = e; overlap = false; return main; }
        used = true;
        return h->aux;
    }
    hipStream_t same() const { return overlap && used ? h->aux : main; }     // right after a get(): the second launch of a pair
    void join()
    {
        if (!used) return;
        hipError_t e = hipEventRecord(h->ev_join, h->aux);
        if (e == hipSuccess) e = hipStreamWaitEvent(main, h->ev_join, 0);
        if (e != hipSuccess) {
            // last resort: the caller's stream cannot be made to wait, so the host waits for the auxiliary stream
            (void)hipStreamSynchronize(h->aux);
            if (err == hipSuccess) err = e;
        }
        used = false;
    }
};

// What a handle call works on.  All pointers null: the descriptors are built for sizing only (make_plan).
struct Ctx {
    unet_handle *h; const Plan &pl; char *base; hipStream_t st;
    const void *const *params; void *const *grads;
    WgradStream wst;
    Ctx(unet_handle *h, const Plan &pl, void *workspace, void *stream, const void *const *params, void *const *grads, bool overlap = false)
        : h(h), pl(pl), base((char *)workspace), st((hipStream_t)stream), params(params), grads(grads), wst{h, st, overlap, false} {}
    float *ws(size_t off) const { return base ? (float *)(base + off) : nullptr; }
    const float *w(int layer) const { return params ? (const float *)params[2 * layer] : nullptr; }
    const float *b(int layer) const { return params ? (const float *)params[2 * layer + 1] : nullptr; }
    float *dw(int layer) const { return grads ? (float *)grads[2 * layer] : nullptr; }
    float *db(int layer) const { return grads ? (float *)grads[2 * layer + 1] : nullptr; }
};

// Weight-gradient launches of a layer (none for conv11c and the head, whose kernels do their own; two over the virtual
// concat, the bias gradient riding on the full-window one).  The slab is sized from these same descriptors.
static int layer_wgrad(const Ctx &cx, int layer, WgradP w[2])
{
    const Plan &pl = cx.pl;
    const Layer &L = LAYERS[layer];
    if (L.kind == K_CONV1 || L.kind == K_HEAD) return 0;
    const Act &x = pl.in(L), &y = pl.out(L);
    const float *dz = cx.ws(y.g);
    float *dw = cx.dw(layer), *db = cx.db(layer), *slab = cx.ws(pl.slab);
    if (L.kind == K_UP) w[0] = upconv_wgrad_desc(cx.ws(x.off), x.e, x.c, dz, y.c, pl.B, dw, slab, pl.slab_bytes, db);
    if (L.kind == K_CONV) w[0] = conv_wgrad_desc(cx.ws(x.off), x.e, x.c, 0, dz, y.e, y.c, pl.B, dw, x.c, 0, slab, pl.slab_bytes, db);
    if (L.kind != K_CAT) return 1;
    const Act &u = pl.u[L.level];
    w[0] = conv_wgrad_desc(cx.ws(x.off), x.e, x.c, pl.pad[L.level], dz, y.e, y.c, pl.B, dw, x.c + u.c, 0, slab, pl.slab_bytes);
    w[1] = conv_wgrad_desc(cx.ws(u.off), u.e, u.c, 0, dz, y.e, y.c, pl.B, dw, x.c + u.c, x.c, slab, pl.slab_bytes, db);
    return 2;
}

static int make_plan(Plan &pl, int base, int B, int S, int training, int math, int ncls = 2)
{
    int rc = check_size(S);
    if (rc) return rc;
    if (B <= 0) { set_error("batch must be positive"); return UNET_E_BADARG; }
    pl = Plan();
    pl.B = B; pl.S = S; pl.base = base; pl.training = training; pl.math = math; pl.ncls = ncls;
    MathScope ms(math);                      // the slab sizing below builds weight-gradient descriptors
    for (int l = 0; l < 5; ++l) pl.ch[l] = base << l;
    Act *acts[26];                           // in allocation order
    int n = 0, cur = S;
    for (int l = 0; l < 5; ++l) {
        pl.a1[l].e = cur - 2; pl.a2[l].e = cur - 4;
        pl.a1[l].c = pl.a2[l].c = pl.ch[l];
        acts[n++] = &pl.a1[l]; acts[n++] = &pl.a2[l];
        if (l < 4) cur = pl.a2[l].e / 2;
    }
    int d = pl.a2[4].e;
    for (int l = 3; l >= 0; --l) {
        pl.t[l].e = pl.a2[l].e / 2;
        pl.u[l].e = 2 * d; pl.pad[l] = (pl.u[l].e - pl.t[l].e) / 2;
        // pad > 0: the skip is zero-padded (every S >= 380); pad < 0: it is cropped (188 <= S < 380).
        // Both are the reference's F.pad(A, (-c,)*4) with c = int((A-B)/2) (network.py:124-126).
        if ((pl.u[l].e - pl.t[l].e) % 2) { set_error("internal: odd skip difference"); return UNET_E_BADSIZE; }
        pl.d1[l].e = pl.u[l].e - 2; pl.d2[l].e = pl.u[l].e - 4; d = pl.d2[l].e;
        pl.t[l].c = pl.u[l].c = pl.d1[l].c = pl.d2[l].c = pl.ch[l];
    }
    for (int l = 0; l < 4; ++l) { acts[n++] = &pl.t[l]; acts[n++] = &pl.u[l]; acts[n++] = &pl.d1[l]; acts[n++] = &pl.d2[l]; }
    pl.So = d;
    if (math == 2 && base % 64 != 0) { set_error("arithmetic mode 2 (bf16 tensors) needs base_ch %% 64 == 0 (got %d)", base); return UNET_E_UNSUPPORTED; }
    // element size of activations, their gradients and the packed filters: bf16 in mode 2, else fp32
    const size_t es = math == 2 ? 2 : 4;
    size_t off = 0;
    auto take_b = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    auto take = [&](size_t elems) { return take_b(elems * es); };
    auto sq = [&](int e, int c) { return (size_t)B * e * e * c; };
    for (int i = 0; i < n; ++i) acts[i]->off = take(sq(acts[i]->e, acts[i]->c));
    for (int i = 0; i < UNET_N_LAYERS; ++i) pl.wt_fwd[i] = take(layer_numel(base, i, false, ncls));
    for (int i = 0; i < UNET_N_LAYERS; ++i) pl.wu_fwd[i] = take_b(math == 3 ? layer_wino_floats(base, i) * 4 : 0);
    if (training) {
        pl.xin = take_b((size_t)B * S * S * 4);
        for (int i = 0; i < UNET_N_LAYERS; ++i) pl.wt_bwd[i] = take(layer_numel(base, i, false, ncls));
        for (int i = 0; i < UNET_N_LAYERS; ++i) pl.wu_bwd[i] = take_b(math == 3 ? layer_wino_floats(base, i) * 4 : 0);
        for (int i = 0; i < n; ++i) {
            Act *a = acts[i];
            a->g = take(sq(a->e, a->c));
            if (a >= pl.t && a < pl.t + 4) pl.g_ts[a - pl.t] = take(sq(a->e, a->c));
        }
        // split-K slab: the largest need over all weight-gradient launches
        size_t need = 0;
        const Ctx sizing(nullptr, pl, nullptr, nullptr, nullptr, nullptr);
        for (int i = 0; i < UNET_N_LAYERS; ++i) {
            WgradP w[2];
            const int nw = layer_wgrad(sizing, i, w);
            for (int j = 0; j < nw; ++j) { const size_t s = wgrad_slab_need(w[j]); if (s > need) need = s; }
        }
        pl.slab_bytes = need;
        pl.slab = take_b(need);
        // small scratch: bias-grad partials, conv11c / head partials
        size_t sm = 0;
        auto upds = [&](size_t s) { if (s > sm) sm = s; };
        for (int l = 0; l < 5; ++l) { upds(bias_grad_scratch_bytes(sq(pl.a1[l].e, 1), pl.ch[l])); upds(bias_grad_scratch_bytes(sq(pl.a2[l].e, 1), pl.ch[l])); }
        for (int l = 0; l < 4; ++l) { upds(bias_grad_scratch_bytes(sq(pl.u[l].e, 1), pl.ch[l])); upds(bias_grad_scratch_bytes(sq(pl.d1[l].e, 1), pl.ch[l])); }
        upds(unet_conv1ch_bwd_scratch_bytes(B, S, base));
        upds(headk_bwd_scratch_bytes(B, pl.So, pl.So, base, ncls));
        pl.small_bytes = sm;
        pl.small = take_b(sm + 4);
    }
    pl.total = off;
    return 0;
}

}  // namespace unet

// =================================================================================================
extern "C" {

const char *unet_last_error(void) { return g_err; }
int unet_abi_version(void) { return 4; }

int unet_set_math(int mode)
{
    ARG_CHECK(mode >= 0 && mode <= 3, "unet_set_math: mode must be 0 (fp32 MFMA), 1 (bf16x3), 2 (bf16) or 3 (fp32 Winograd)");
    set_math_mode(mode);
    return 0;
}
int unet_get_math(void) { return get_math_mode(); }

int unet_set_lds_dma(int mode)
{
    ARG_CHECK(mode == 0 || mode == 1, "unet_set_lds_dma: mode must be 0 (global_load_lds) or 1 (buffer descriptors when tensors fit)");
    set_lds_dma_mode(mode);
    return 0;
}

// the device a call must run on: the handle's.  Everything the library keeps per device (zero page, LDS attributes) is
// keyed on hipGetDevice(), so a call made while another device is current would enqueue on the wrong device.
#define CHECK_DEVICE(h, what)                                                                                          \
    do {                                                                                                               \
        int cur_ = -1;                                                                                                 \
        HIP_TRY(hipGetDevice(&cur_));                                                                                  \
        ARG_CHECK(cur_ == (h)->device, what ": the handle belongs to device %d but device %d is current "               \
                  "(one process per GPU: hipSetDevice / torch.cuda.set_device first)", (h)->device, cur_);             \
    } while (0)

int unet_create(unet_handle **out, const unet_config *cfg) { return unet_create_classes(out, cfg, 2); }

int unet_create_classes(unet_handle **out, const unet_config *cfg, int n_classes)
{
    ARG_CHECK(out && cfg, "unet_create: null argument");
    ARG_CHECK(n_classes >= 2 && n_classes <= UNET_MAX_CLASSES, "unet_create_classes: n_classes %d unsupported (2..%d)", n_classes,
              UNET_MAX_CLASSES);
    ARG_CHECK(cfg->base_ch == 64 || cfg->base_ch == 32, "unet_create: base_ch %d unsupported (32 or 64)", cfg->base_ch);
    ARG_CHECK(cfg->math >= -1 && cfg->math <= 3, "unet_create: math %d unsupported (-1 = process default, 0..3)", cfg->math);
    // the zero page is made on the handle's device; the caller's current device is left as it was
    int prev = -1;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(cfg->device));
    const bool ok = zero_page() != nullptr;
    HIP_TRY(hipSetDevice(prev));
    if (!ok) return UNET_E_BADARG;
    unet_handle *h = new unet_handle();
    h->base_ch = cfg->base_ch;
    h->device = cfg->device;
    h->math = cfg->math;
    h->n_classes = n_classes;
    *out = h;
    return 0;
}

int unet_n_classes(const unet_handle *h) { return h ? h->n_classes : 0; }

int unet_destroy(unet_handle *h)
{
    if (h && h->dp) (void)unet_dp_free(h->dp);
    if (h) {
        if (h->aux) { (void)hipStreamSynchronize(h->aux); (void)hipStreamDestroy(h->aux); }
        if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
        if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    }
    delete h;
    return 0;
}

int unet_set_grad_scale(unet_handle *h, float scale)
{
    ARG_CHECK(h, "unet_set_grad_scale: null handle");
    ARG_CHECK(scale > 0.f && scale <= 1.f, "unet_set_grad_scale: scale must be in (0, 1] (1/world), got %g", (double)scale);
    h->grad_scale = scale;
    return 0;
}

// -1 (default): by what was measured - on with bf16 tensors (+2.6 ... +3 % per step: the weight gradients fill the dgrad chain's
// partial rounds) and in fp32 at batches of <= 4 tiles (+0.2 ... +1.2 %), off in fp32 at larger batches (-0.6 ... -1 % at B = 8: the
// co-running fp32 MFMA kernels slow each other by more)
static int g_overlap = [] { const char *e = getenv("UNET_OVERLAP"); return e ? atoi(e) : -1; }();
int unet_set_overlap(int on)
{
    ARG_CHECK(on >= -1 && on <= 1, "unet_set_overlap: -1 (per arithmetic mode), 0 or 1");
    g_overlap = on;
    return 0;
}

static int handle_math(const unet_handle *h) { return h->math >= 0 ? h->math : get_math_mode(); }

int unet_output_size(int S, int *out_size)
{
    int rc = check_size(S);
    if (rc) return rc;
    if (out_size) *out_size = S - 184;
    return 0;
}

int unet_param_count(const unet_handle *h, int idx, size_t *numel)
{
    ARG_CHECK(h && numel && idx >= 0 && idx < UNET_N_PARAMS, "unet_param_count: bad argument");
    *numel = layer_numel(h->base_ch, idx / 2, idx & 1, h->n_classes);
    return 0;
}

size_t unet_workspace_bytes(const unet_handle *h, int B, int S, int training)
{
    if (!h) { set_error("null handle"); return 0; }
    Plan pl;
    if (make_plan(pl, h->base_ch, B, S, training, handle_math(h), h->n_classes)) return 0;
    return pl.total;
}

double unet_flops(const unet_handle *h, int B, int S, int backward)
{
    if (!h) return 0.0;
    Plan pl;
    if (make_plan(pl, h->base_ch, B, S, 0, handle_math(h), h->n_classes)) return 0.0;
    double f = 0.0, f11c = 0.0, first = 0.0;
    for (int i = 0; i < UNET_N_LAYERS; ++i) {
        const Layer &L = LAYERS[i];
        const int k = layer_taps(L);
        // pixels the filter is applied at: the output's, for the up-conv (and the head) the input's
        const int eo = L.kind == K_UP || L.kind == K_HEAD ? pl.in(L).e : pl.out(L).e;
        const double a = 2.0 * B * (double)eo * eo * layer_ci(pl.base, L) * layer_co(pl.base, L, pl.ncls) * k * k;
        if (L.kind == K_CONV1) f11c = a;
        // (order of summation: the two convs of a level are added to each other first)
        if (L.out == T_A1 || L.out == T_D1) first = a;
        else if (L.out == T_A2 || L.out == T_D2) f += first + a;
        else f += a;
    }
    return backward ? 3.0 * f - f11c : f;      // bwd = dgrad + wgrad, conv11c needs no dgrad (A23)
}

static int pool_launch(const Ctx &cx, int l, bool bwd)
{
    char nm[40]; snprintf(nm, sizeof(nm), "pool%d.%s", l + 1, bwd ? "bwd" : "fwd");
    ProfScope ps(nm);
    const Act &a2 = cx.pl.a2[l], &t = cx.pl.t[l];
    return bwd ? maxpool2_bwd(cx.ws(a2.off), cx.ws(t.g), cx.ws(a2.g), cx.pl.B, a2.e, a2.e, a2.c, t_es, cx.st)
               : maxpool2_fwd(cx.ws(a2.off), cx.ws(t.off), cx.pl.B, a2.e, a2.e, a2.c, t_es, cx.st);
}

// Drop-out of a layer's output where the table has a site (and the forward was planned with p > 0).  Forward: in place, and
// where the output is pooled the pooled tensor t[l] of the dropped values.  Backward: the output's gradient times 1 / (1 - p);
// every consumer has already masked it with (dropped tensor > 0), and a dropped element is exactly 0 there.
static int drop_launch(const Ctx &cx, int layer, bool bwd)
{
    const Plan &pl = cx.pl;
    const Layer &L = LAYERS[layer];
    char nm[40]; snprintf(nm, sizeof(nm), "drop%d.%s", L.level + 1, bwd ? "bwd" : "fwd");
    ProfScope ps(nm);
    const Act &y = pl.out(L);
    if (bwd) return dropout_bwd(cx.ws(y.g), tensor_elems(pl.B, y.e, y.e, y.c), pl.drop_p, t_es, cx.st);
    return dropout_pool_fwd(cx.ws(y.off), L.level < 4 ? cx.ws(pl.t[L.level].off) : nullptr, pl.B, y.e, y.e, y.c, pl.drop_p, pl.drop_seed,
                            pl.drop_step, L.drop, t_es, cx.st);
}

// Forward of a 3x3 layer of the table: K_CONV, or K_CAT over the virtual concat of the padded skip t[l] and u[l].  The
// second conv of an encoder level is followed by the pool, fused into its launch where the Winograd epilogue can.
static int conv_forward(const Ctx &cx, int layer)
{
    const Plan &pl = cx.pl;
    const Layer &L = LAYERS[layer];
    const bool cat = L.kind == K_CAT, pools = L.out == T_A2 && L.level < 4, drops = pl.drops(L);
    const Act &x1 = pl.in(L), &y = pl.out(L), *x2 = cat ? &pl.u[L.level] : nullptr;
    bool pool_fused = false;
    {
        RowScope rs(layer, "fwd");
        int rc = conv_fwd_launch(cx.ws(x1.off), x1.e, x1.c, cat ? pl.pad[L.level] : 0, cat ? cx.ws(x2->off) : nullptr, cat ? x2->c : 0, pl.B, y.e + 2,
                                 cx.w(layer), cx.ws(pl.wt_fwd[layer]), cx.b(layer), y.c, 1, cx.ws(y.off), cx.st, cx.ws(pl.wu_fwd[layer]),
                                 pools && !drops ? cx.ws(pl.t[L.level].off) : nullptr, &pool_fused);
        if (rc) return rc;
    }
    if (drops) return drop_launch(cx, layer, false);     // the pool must see the dropped values: its kernel pools too
    return pools && !pool_fused ? pool_launch(cx, L.level, false) : 0;
}

// unet_forward and unet_forward_dropout (p > 0: the two drop-out sites of the table are active; p == 0 is unet_forward)
static int forward_body(unet_handle *h, const void *const *params, const void *x, void *logits, int B, int S, void *workspace,
                        size_t workspace_bytes, int training, float drop_p, unsigned long long drop_seed, unsigned long long drop_step,
                        void *stream)
{
    ARG_CHECK(h && params && x && logits && workspace, "unet_forward: null argument");
    CHECK_DEVICE(h, "unet_forward");
    Plan pl;
    int rc = make_plan(pl, h->base_ch, B, S, training, handle_math(h), h->n_classes);
    if (rc) return rc;
    pl.drop_p = drop_p; pl.drop_seed = drop_seed; pl.drop_step = drop_step;
    MathScope ms(pl.math);
    ARG_CHECK(workspace_bytes >= pl.total, "unet_forward: workspace too small (%zu < %zu)", workspace_bytes, pl.total);
    ARG_CHECK(((uintptr_t)workspace & 255) == 0, "unet_forward: workspace must be 256-byte aligned");
    const Ctx cx(h, pl, workspace, stream, params, nullptr);
    hipStream_t st = cx.st;
    // whatever plan this address had is void from here on: this forward overwrites the workspace.  A training forward
    // registers its own plan once everything is enqueued; an inference forward leaves none, so a backward on this address
    // is refused (UNET_E_NOTREADY) rather than run over an inference layout.
    h->live.forget(workspace);

    // repack the parameters (reference layout, owned by the caller and updated by its optimizer): the up-convs', level 0 first
    // (the 3x3 layers' weights are packed lazily, only if a launch of the layer takes the implicit-GEMM path: with_wino)
    for (int i = UNET_N_LAYERS - 1; i >= 0; --i) {
        if (LAYERS[i].kind != K_UP) continue;
        RowScope rs(i, "fwd");
        if ((rc = pack_upconv_fwd(cx.w(i), cx.ws(pl.wt_fwd[i]), pl.ch[LAYERS[i].ci], pl.ch[LAYERS[i].co], t_es, st))) return rc;
    }

    // the layers in order: encoder (network.py:131-156), decoder (network.py:159-188: up-conv, virtual zero-pad-concat, two
    // convs), head
    for (int i = 0; i < UNET_N_LAYERS; ++i) {
        const Layer &L = LAYERS[i];
        switch (L.kind) {
        case K_CONV1: {                      // the input is kept for conv11c's weight gradient
            RowScope rs(i, "fwd");
            if (training) HIP_TRY(hipMemcpyAsync(cx.ws(pl.xin), x, (size_t)B * S * S * sizeof(float), hipMemcpyDeviceToDevice, st));
            if ((rc = conv1ch_fwd((const float *)x, B, S, cx.w(i), cx.b(i), pl.ch[0], cx.ws(pl.a1[0].off), t_es, st))) return rc;
            break;
        }
        case K_CONV:
        case K_CAT:
            if ((rc = conv_forward(cx, i))) return rc;
            break;
        case K_UP: {
            RowScope rs(i, "fwd");
            const Act &in = pl.in(L), &u = pl.u[L.level];
            IgemmP p = upconv_fwd_desc(cx.ws(in.off), B, in.e, in.e, in.c, cx.ws(pl.wt_fwd[i]), cx.b(i), u.c, cx.ws(u.off));
            if ((rc = launch_igemm(p, st))) return rc;
            break;
        }
        case K_HEAD: {
            RowScope rs(i, "fwd");
            const Act &in = pl.in(L);
            if ((rc = headk_fwd(cx.ws(in.off), B, in.e, in.e, in.c, pl.ncls, cx.w(i), cx.b(i), (float *)logits, t_es, st))) return rc;
            break;
        }
        }
    }
    if (training) h->live.remember(workspace, pl);
    return 0;
}

int unet_forward(unet_handle *h, const void *const *params, const void *x, void *logits, int B, int S,
                 void *workspace, size_t workspace_bytes, int training, void *stream)
{
    return forward_body(h, params, x, logits, B, S, workspace, workspace_bytes, training, 0.f, 0, 0, stream);
}

int unet_forward_dropout(unet_handle *h, const void *const *params, const void *x, void *logits, int B, int S,
                         void *workspace, size_t workspace_bytes, float p, unsigned long long seed, unsigned long long step, void *stream)
{
    ARG_CHECK(p >= 0.f && p < 1.f, "unet_forward_dropout: p must be in [0, 1), got %g", (double)p);
    return forward_body(h, params, x, logits, B, S, workspace, workspace_bytes, 1, p, seed, step, stream);
}

int unet_activation_bytes(const unet_handle *h)
{
    if (!h) return 0;
    return handle_math(h) == 2 ? 2 : 4;
}

/* Debug/introspection: byte offset and element count of a named workspace buffer, e.g. "a1_0",
 * "a2_4", "t_2", "u_3", "d1_0", "d2_3", and with training=1 "g_a1_0", "g_a2_4", "g_t_1", "g_ts_1",
 * "g_u_2", "g_d1_3", "g_d2_3", "xin".  Tensors are NHWC [B,e,e,C]; extent and channels describe them. */
int unet_debug_buffer(const unet_handle *h, int B, int S, int training, const char *name,
                      size_t *offset, int *extent, int *channels)
{
    ARG_CHECK(h && name && offset && extent && channels, "unet_debug_buffer: null argument");
    Plan pl;
    int rc = make_plan(pl, h->base_ch, B, S, training, handle_math(h), h->n_classes);
    if (rc) return rc;
    char kind[16];
    const char *us = strrchr(name, '_');
    if (!strcmp(name, "xin")) { ARG_CHECK(training, "xin exists only with training=1"); *offset = pl.xin; *extent = S; *channels = 1; return 0; }
    ARG_CHECK(us && (size_t)(us - name) < sizeof(kind), "unet_debug_buffer: bad name %s", name);
    memcpy(kind, name, us - name); kind[us - name] = 0;
    const int l = atoi(us + 1);
    ARG_CHECK(l >= 0 && l < 5, "unet_debug_buffer: bad level in %s", name);
    const bool g = !strncmp(kind, "g_", 2);
    ARG_CHECK(!g || training, "gradient buffers exist only with training=1");
    const char *k = g ? kind + 2 : kind;
    const bool ts = g && !strcmp(k, "ts");                  // the one buffer that is no tensor's gradient: t's extent
    int id = ts ? T_T : 0;
    while (!ts && id < N_TENSORS && strcmp(k, TENSOR_NAME[id].name)) ++id;
    ARG_CHECK(l < (id < N_TENSORS ? TENSOR_NAME[id].levels : 4), "unet_debug_buffer: bad level in %s", name);
    if (id == N_TENSORS) { set_error("unet_debug_buffer: unknown buffer %s", name); return UNET_E_BADARG; }
    const Act &a = pl.act(id, l);
    *offset = ts ? pl.g_ts[l] : g ? a.g : a.off; *extent = a.e; *channels = a.c;
    return 0;
}

// ---- backward ------------------------------------------------------------------------------------
// (stages: the table's column; a stage's layers run last first)
int unet_backward_stages(void) { return N_STAGES; }

int unet_backward_stage_params(int stage, int *idx, int cap)
{
    int k = 0;
    for (int i = UNET_N_LAYERS - 1; i >= 0; --i)
        for (int b = 0; b < 2 && LAYERS[i].stage == stage; ++b, ++k)
            if (idx && k < cap) idx[k] = 2 * i + b;
    return k;
}

// weight gradient (+ bias gradient) of a layer, next to the dgrad chain when the stage overlaps
static int wgrad_backward(Ctx &cx, int layer)
{
    RowScope rs(layer, "wgrad");
    WgradP w[2];
    const int n = layer_wgrad(cx, layer, w);
    for (int j = 0; j < n; ++j) {
        int rc = launch_wgrad(w[j], j ? cx.wst.same() : cx.wst.get());
        if (rc) return rc;
    }
    return 0;
}

// Single-source 3x3 conv: wgrad + bias grad, dgrad.  Its input is a ReLU output, which masks the dgrad - or the pool's t[l]:
// then the skip's gradient g_ts[l] is added instead and the pool's backward follows.
static int conv_backward(Ctx &cx, int layer)
{
    const Plan &pl = cx.pl;
    const Layer &L = LAYERS[layer];
    const Act &x = pl.in(L), &y = pl.out(L);
    const bool pooled = L.in == T_T;
    int rc;
    // drop-out site: the output's gradient is scaled on the caller's stream before the weight gradient forks from it, so
    // that both it and the dgrad read the scaled tensor
    if (pl.drops(L) && (rc = drop_launch(cx, layer, true))) return rc;
    if ((rc = wgrad_backward(cx, layer))) return rc;
    {
        RowScope rs(layer, "dgrad");
        if ((rc = conv_dgrad_launch(cx.ws(y.g), y.e, y.c, pl.B, cx.w(layer), cx.ws(pl.wt_bwd[layer]), cx.ws(pl.wu_bwd[layer]), x.e, x.c, 0, cx.ws(x.g),
                                    pooled ? nullptr : cx.ws(x.off), pooled ? cx.ws(pl.g_ts[L.ci]) : nullptr, 0, 0, nullptr, nullptr, cx.st))) return rc;
    }
    return pooled ? pool_launch(cx, L.ci, true) : 0;
}

// the layers of a stage, last first
static int backward_stage_body(Ctx &cx, int stage, const void *dlogits)
{
    const Plan &pl = cx.pl;
    hipStream_t st = cx.st;
    const int B = pl.B;
    int rc;
    for (int i = UNET_N_LAYERS - 1; i >= 0; --i) {
        const Layer &L = LAYERS[i];
        if (L.stage != stage) continue;
        switch (L.kind) {
        case K_HEAD: {                       // fused with the ReLU backward of conv12e -> dz of conv12e
            ARG_CHECK(dlogits, "unet_backward: null dlogits");
            RowScope rs(i, "bwd");
            const Act &x = pl.in(L);
            if ((rc = headk_bwd(cx.ws(x.off), B, x.e, x.e, x.c, pl.ncls, cx.w(i), (const float *)dlogits, cx.h->grad_scale, cx.ws(x.g),
                                cx.dw(i), cx.db(i), cx.ws(pl.small), t_es, st))) return rc;
            break;
        }
        case K_CONV:
            if ((rc = conv_backward(cx, i))) return rc;
            break;
        case K_CAT: {                        // virtual concat input: dgrad per source half (skip half only over the crop window)
            const int l = L.level;
            const Act &t = pl.t[l], &u = pl.u[l], &y = pl.d1[l];
            if ((rc = wgrad_backward(cx, i))) return rc;
            RowScope rs(i, "dgrad");
            if ((rc = conv_dgrad_launch(cx.ws(y.g), y.e, y.c, B, cx.w(i), cx.ws(pl.wt_bwd[i]), cx.ws(pl.wu_bwd[i]), t.e, t.c, pl.pad[l], cx.ws(pl.g_ts[l]), nullptr, nullptr,
                                        u.e, u.c, cx.ws(u.g), nullptr, st))) return rc;
            break;
        }
        case K_UP: {                         // its input is a ReLU output (d2[l+1] or a2[4]), which masks its dgrad
            const Act &x = pl.in(L), &u = pl.u[L.level];
            if ((rc = wgrad_backward(cx, i))) return rc;
            RowScope rs(i, "dgrad");
            if ((rc = pack_upconv_dgrad(cx.w(i), cx.ws(pl.wt_bwd[i]), x.c, u.c, t_es, st))) return rc;
            IgemmP d = upconv_dgrad_desc(cx.ws(u.g), B, x.e, x.e, x.c, cx.ws(pl.wt_bwd[i]), u.c, cx.ws(x.g), cx.ws(x.off));
            if ((rc = launch_igemm(d, st))) return rc;
            break;
        }
        case K_CONV1: {                      // weight/bias gradient only (A1 needs no dgrad)
            RowScope rs(i, "wgrad");
            if ((rc = conv1ch_bwd(cx.ws(pl.xin), B, pl.S, pl.ch[0], cx.ws(pl.a1[0].g), cx.dw(i), cx.db(i), cx.ws(pl.small), t_es, st))) return rc;
            break;
        }
        }
    }
    return 0;
}

int unet_backward_stage(unet_handle *h, int stage, const void *const *params, const void *dlogits, void *const *grads,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    ARG_CHECK(h && params && grads && workspace, "unet_backward: null argument");
    CHECK_DEVICE(h, "unet_backward");
    Plan pl;
    if (!h->live.lookup(workspace, pl)) {
        set_error("unet_backward: this handle has no training forward planned on this workspace address (none was run there, "
                  "or an inference forward has overwritten it since)");
        return UNET_E_NOTREADY;
    }
    ARG_CHECK(workspace_bytes >= pl.total, "unet_backward: workspace too small");
    ARG_CHECK(stage >= 0 && stage < N_STAGES, "unet_backward: bad stage %d", stage);
    MathScope ms(pl.math);                   // the arithmetic the forward was planned with
    // (no overlap while per-launch events are recorded: launches of two streams would interleave their begin / end events)
    // (fp32 at batches of <= 4 tiles: the deep layers' launches leave CUs idle that the weight gradients can take: +0.7 % at B = 2,
    //  +1.2 % at B = 1; at B = 8 the two families only get in each other's way)
    const bool overlap = (g_overlap < 0 ? (pl.math == 2 || pl.B <= 4) : g_overlap != 0) && !prof_active();
    if (overlap && !h->aux) {
        HIP_TRY(hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    }
    Ctx cx(h, pl, workspace, stream, params, grads, overlap);
    int rc = backward_stage_body(cx, stage, dlogits);
    cx.wst.join();                           // every path re-joins the streams before the caller sees the stage as enqueued
    if (rc == 0 && cx.wst.err != hipSuccess) {
        set_error("unet_backward: ordering the weight-gradient stream against the caller's failed: %s", hipGetErrorString(cx.wst.err));
        rc = (int)cx.wst.err;
    }
    // the forward's backward has been enqueued in full: its plan no longer holds a place among the pending ones (it stays
    // readable for unet_backward_input and a repeated backward until newer finished plans push it out)
    if (rc == 0 && stage == N_STAGES - 1) h->live.finish(workspace);
    return rc;
}

int unet_backward_input(unet_handle *h, const void *const *params, void *dx, void *workspace, size_t workspace_bytes, void *stream)
{
    ARG_CHECK(h && params && dx && workspace, "unet_backward_input: null argument");
    CHECK_DEVICE(h, "unet_backward_input");
    Plan pl;
    if (!h->live.lookup(workspace, pl)) {
        set_error("unet_backward_input: this handle has no training forward planned on this workspace address (none was run "
                  "there, or an inference forward has overwritten it since)");
        return UNET_E_NOTREADY;
    }
    ARG_CHECK(workspace_bytes >= pl.total, "unet_backward_input: workspace too small");
    MathScope ms(pl.math);
    const Ctx cx(h, pl, workspace, stream, params, nullptr);
    RowScope rs(C11C, "dgrad");
    // g_a1[0] = d loss / d conv11c's output, masked by its ReLU: final once the last backward stage has been enqueued
    return conv1ch_dgrad(cx.ws(pl.a1[0].g), pl.B, pl.S, pl.ch[0], cx.w(C11C), (float *)dx, t_es, cx.st);
}

int unet_backward(unet_handle *h, const void *const *params, const void *dlogits, void *const *grads,
                  void *workspace, size_t workspace_bytes, void *stream)
{
    for (int s = 0; s < N_STAGES; ++s) {
        int rc = unet_backward_stage(h, s, params, dlogits, grads, workspace, workspace_bytes, stream);
        if (rc) return rc;
    }
    return 0;
}

// Upper bound of the split-K slab for the per-op entry point (the split of C into two sources and the
// skip window are not known when the caller sizes its scratch): twice the larger full-window need.
static size_t conv_bwd_slab_bound(int B, int H, int C, int K)
{
    size_t need = 0;
    for (int math = 0; math <= 2; math += 2) {          // the decomposition differs between the fp32 and the bf16 kernels
        MathScope ms(math);
        for (int ci = 64; ci <= (C + 63) / 64 * 64; ci *= 2) {
            WgradP w = conv_wgrad_desc(nullptr, H, ci, 0, nullptr, H - 2, K, B, nullptr, ci, 0, nullptr, 0);
            const size_t n = wgrad_slab_need(w);
            if (n > need) need = n;
        }
    }
    return align_up(2 * need, 256);
}

static size_t upconv_slab_bound(int B, int H, int Ci, int Co)
{
    size_t need = 0;
    for (int math = 0; math <= 2; math += 2) {
        MathScope ms(math);
        WgradP w = upconv_wgrad_desc(nullptr, H, Ci, nullptr, Co, B, nullptr, nullptr, 0);
        const size_t n = wgrad_slab_need(w);
        if (n > need) need = n;
    }
    return align_up(need, 256);
}

// ---- per-op entry points (unit tests) --------------------------------------------------------------
static size_t wino_scratch_bytes(int C, int K)
{
    // U of a per-op call, whole 64-row blocks (wino_u_floats): forward 16 C rup64(K) (the sources' sub-matrices add up to it);
    // dgrad one sub-matrix per source, 16 K (rup64(C1) + rup64(C2)) <= 16 K (rup64(C) + 64)
    const size_t fwd = wino_u_floats(C, K), bwd = wino_u_floats(K, C) + wino_u_floats(K, 64);
    return align_up((fwd > bwd ? fwd : bwd) * sizeof(float), 256);
}
// The one size rule (common.hpp) for one tensor of a per-op 3x3 call, checked before anything is enqueued (what launch_igemm /
// launch_igemmb / launch_wgrad would refuse after the filters have been packed): fewer than 2^31 - 1 elements, and a bf16
// tensor that a kernel stages (`staged`: the bf16 kernels have buffer-descriptor staging only) fewer than 2^31 - 1 bytes.
// The launchers keep their own checks (the net's path goes through them alone); this one only moves the refusal in front of
// the first enqueue.  `staged` at the call sites follows who reads the tensor as a source:
//   forward   x1, x2: launch_igemmb (igemm_source_bytes);  y: a destination, never staged
//   backward  dz: launch_igemmb for each dgrad that runs (dx1, dx2) and launch_wgrad_b (its Y) when dw is asked for;
//             x1, x2: launch_wgrad_b (its X), so only with dw;  the stand-alone bias_grad takes dz at any size
static int op_tensor_ok(const char *op, const char *name, int B, int H, int W, int C, bool staged)
{
    const size_t n = tensor_elems(B, H, W, C);
    ARG_CHECK(n < LIMIT_31BIT, "%s: %s [%d,%d,%d,%d] has %zu elements, the limit is 2^31 - 1 = %zu (31-bit element offsets)", op, name, B, H, W, C, n, LIMIT_31BIT);
    ARG_CHECK(!(staged && t_math == 2) || fits_buffer(n * 2), "%s: bf16 %s [%d,%d,%d,%d] has %zu bytes, the limit is 2^31 - 1 = %zu (2 GiB: buffer-descriptor staging)",
              op, name, B, H, W, C, n * 2, LIMIT_31BIT);
    return 0;
}

size_t unet_conv3x3_scratch_bytes(int C, int K) { return align_up((size_t)K * C * 9 * sizeof(float), 256) + wino_scratch_bytes(C, K); }

int unet_conv3x3_fwd(const void *x1, int H1, int W1, int C1, int pad1, const void *x2, int C2, int B, int H, int W,
                     const void *w_oihw, const void *bias, int K, int relu, void *y, void *scratch, void *stream)
{
    ARG_CHECK(x1 && w_oihw && y && scratch, "conv3x3_fwd: null argument");
    MathScope ms(get_math_mode());
    ProfScope ps("op.conv3x3_fwd");
    ARG_CHECK(x2 || (H1 + 2 * pad1 == H && W1 + 2 * pad1 == W), "conv3x3_fwd: single source must match the input extent");
    hipStream_t st = (hipStream_t)stream;
    ARG_CHECK(H == W && H1 == W1, "conv3x3_fwd: square tiles only");
    // (what launch_igemmb would refuse after the filters have been packed: refused here, before anything is enqueued)
    ARG_CHECK(t_math != 2 || (C1 % 64 == 0 && (!x2 || C2 % 64 == 0)), "conv3x3_fwd: bf16 tensors need sources of whole 64-channel tiles (C1=%d C2=%d)", C1, x2 ? C2 : 0);
    int rc;
    if ((rc = op_tensor_ok("conv3x3_fwd", "x1", B, H1, W1, C1, true))) return rc;
    if (x2 && (rc = op_tensor_ok("conv3x3_fwd", "x2", B, H, W, C2, true))) return rc;
    if ((rc = op_tensor_ok("conv3x3_fwd", "y", B, H - 2, W - 2, K, false))) return rc;
    float *wu = (float *)((char *)scratch + align_up((size_t)K * (C1 + (x2 ? C2 : 0)) * 9 * sizeof(float), 256));
    return conv_fwd_launch((const float *)x1, H1, C1, pad1, (const float *)x2, C2, B, H, (const float *)w_oihw, (float *)scratch,
                           (const float *)bias, K, relu, (float *)y, st, wu);
}

size_t unet_conv3x3_bwd_scratch_bytes(int B, int H, int W, int C, int K)
{
    return align_up((size_t)K * C * 9 * sizeof(float), 256) + conv_bwd_slab_bound(B, H, C, K) +
           align_up(bias_grad_scratch_bytes((size_t)B * (H - 2) * (W - 2), K), 256) + wino_scratch_bytes(C, K);
}

int unet_conv3x3_bwd(const void *x1, int H1, int W1, int C1, int pad1, const void *x2, int C2, int B, int H, int W,
                     const void *w_oihw, int K, const void *dz, void *dx1, const void *mask1, const void *add1,
                     void *dx2, const void *mask2, void *dw, void *db, void *scratch, void *stream)
{
    ARG_CHECK(x1 && w_oihw && dz && scratch, "conv3x3_bwd: null argument");
    MathScope ms(get_math_mode());
    ProfScope ps("op.conv3x3_bwd");
    ARG_CHECK(x2 || (H1 + 2 * pad1 == H && W1 + 2 * pad1 == W), "conv3x3_bwd: single source must match the input extent");
    ARG_CHECK(H == W && H1 == W1, "conv3x3_bwd: square tiles only");
    // (what launch_igemmb / launch_wgrad would refuse after the first launches: refused here, before anything is enqueued)
    if (t_math == 2) {
        ARG_CHECK(!(dx1 || (x2 && dx2) || dw) || K % 64 == 0, "conv3x3_bwd: bf16 tensors need dz of whole 64-channel tiles (K=%d)", K);
        ARG_CHECK(!dw || (C1 % 64 == 0 && (!x2 || C2 % 64 == 0)), "conv3x3_bwd: the bf16 weight gradient needs sources of whole 64-channel tiles (C1=%d C2=%d)",
                  C1, x2 ? C2 : 0);
    }
    int rc;
    if ((rc = op_tensor_ok("conv3x3_bwd", "x1", B, H1, W1, C1, dw != nullptr))) return rc;
    if (x2 && (rc = op_tensor_ok("conv3x3_bwd", "x2", B, H, W, C2, dw != nullptr))) return rc;
    if ((rc = op_tensor_ok("conv3x3_bwd", "dz", B, H - 2, W - 2, K, dx1 || (x2 && dx2) || dw))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int C = C1 + (x2 ? C2 : 0);
    const int Ho = H - 2;
    float *wt = (float *)scratch;
    const size_t wt_bytes = align_up((size_t)K * C * 9 * sizeof(float), 256);
    const size_t slab_bytes = conv_bwd_slab_bound(B, H, C, K);
    float *slab = (float *)((char *)scratch + wt_bytes);
    float *small = (float *)((char *)scratch + wt_bytes + slab_bytes);
    float *wu = (float *)((char *)scratch + wt_bytes + slab_bytes + align_up(bias_grad_scratch_bytes((size_t)B * Ho * Ho, K), 256));
    if ((rc = conv_dgrad_launch((const float *)dz, Ho, K, B, (const float *)w_oihw, wt, wu, H1, C1, pad1, (float *)dx1, (const float *)mask1,
                                (const float *)add1, H, C - C1, x2 ? (float *)dx2 : nullptr, (const float *)mask2, st))) return rc;
    bool db_done = false;
    if (dw) {
        // the bias gradient rides on whichever weight-gradient launch covers the full dz window
        const bool full1 = !x2 && pad1 == 0;
        WgradP w1 = conv_wgrad_desc((const float *)x1, H1, C1, pad1, (const float *)dz, Ho, K, B, (float *)dw, C, 0, slab, slab_bytes,
                                    full1 ? (float *)db : nullptr);
        if ((rc = launch_wgrad(w1, st))) return rc;
        db_done = full1 && db;
        if (x2) {
            WgradP w2 = conv_wgrad_desc((const float *)x2, H, C2, 0, (const float *)dz, Ho, K, B, (float *)dw, C, C1, slab, slab_bytes, (float *)db);
            if ((rc = launch_wgrad(w2, st))) return rc;
            db_done = db != nullptr;
        }
    }
    if (db && !db_done && (rc = bias_grad(dz, (size_t)B * Ho * Ho, K, (float *)db, small, t_es, st))) return rc;
    return 0;
}

size_t unet_upconv2_scratch_bytes(int B, int H, int W, int Ci, int Co)
{
    (void)W;
    return align_up((size_t)Ci * Co * 4 * sizeof(float), 256) + upconv_slab_bound(B, H, Ci, Co) +
           align_up(bias_grad_scratch_bytes((size_t)B * 4 * H * W, Co), 256);
}

int unet_upconv2_fwd(const void *x, int B, int H, int W, int Ci, const void *w_iohw, const void *bias, int Co,
                     void *y, void *scratch, void *stream)
{
    ARG_CHECK(x && w_iohw && y && scratch, "upconv2_fwd: null argument");
    MathScope ms(get_math_mode());
    ProfScope ps("op.upconv2_fwd");
    hipStream_t st = (hipStream_t)stream;
    int rc = pack_upconv_fwd((const float *)w_iohw, scratch, Ci, Co, t_es, st);
    if (rc) return rc;
    return launch_igemm(upconv_fwd_desc((const float *)x, B, H, W, Ci, (const float *)scratch, (const float *)bias, Co, (float *)y), st);
}

int unet_upconv2_bwd(const void *x, int B, int H, int W, int Ci, const void *w_iohw, int Co, const void *dy,
                     void *dx, const void *mask, void *dw, void *db, void *scratch, void *stream)
{
    ARG_CHECK(x && w_iohw && dy && scratch, "upconv2_bwd: null argument");
    ARG_CHECK(H == W, "upconv2_bwd: square tiles only");
    MathScope ms(get_math_mode());
    ProfScope ps("op.upconv2_bwd");
    hipStream_t st = (hipStream_t)stream;
    float *wt = (float *)scratch;
    const size_t wt_bytes = align_up((size_t)Ci * Co * 4 * sizeof(float), 256);
    const size_t slab_bytes = upconv_slab_bound(B, H, Ci, Co);
    float *slab = (float *)((char *)scratch + wt_bytes);
    float *small = (float *)((char *)scratch + wt_bytes + slab_bytes);
    int rc;
    if (dx) {
        if ((rc = pack_upconv_dgrad((const float *)w_iohw, wt, Ci, Co, t_es, st))) return rc;
        if ((rc = launch_igemm(upconv_dgrad_desc((const float *)dy, B, H, W, Ci, wt, Co, (float *)dx, (const float *)mask), st))) return rc;
    }
    if (dw) {
        WgradP w = upconv_wgrad_desc((const float *)x, H, Ci, (const float *)dy, Co, B, (float *)dw, slab, slab_bytes, (float *)db);
        if ((rc = launch_wgrad(w, st))) return rc;
    } else if (db && (rc = bias_grad(dy, (size_t)B * 4 * H * W, Co, (float *)db, small, t_es, st))) return rc;
    return 0;
}

}  // extern "C"
