// conv_mfma.hip -- dispatch of the NHWC float32 convolution kernels (conv_f32.hip: exact-f32 MFMA; conv_bx3.hip /
// conv_h2.hip / conv_h2d.hip: split-precision kernels on the 16-bit matrix pipe) + the naive bring-up cross-check.
#include "conv_common.h"
#include <mutex>
#include <vector>

namespace romp {

// Bring-up cross-check: one thread per output element, same packed weights, plain FMA loop.
__global__ void conv_naive_kernel(ConvParams p, int KS, int S, int B, int groups) {
    const size_t total = (size_t)B * p.Ho * p.Wo * p.Cout * groups;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        size_t r = t;
        const int co = r % p.Cout; r /= p.Cout;
        const int g = r % groups; r /= groups;
        const int ox = r % p.Wo; r /= p.Wo;
        const int oy = r % p.Ho;
        const int b = r / p.Ho;
        const float* in = p.in + (size_t)b * p.H * p.W * p.in_cs + p.in_co + g * p.in_gs;
        const float* wg = p.w + (size_t)g * p.w_gs;
        const int KH = KS == 13 ? 1 : KS, KW = KS == 13 ? 3 : KS;
        float acc = 0.f;
        for (int tap = 0; tap < KH * KW; ++tap) {
            const int iy = oy * S - p.pad_h + tap / KW, ix = ox * S - p.pad_w + tap % KW;
            if ((unsigned)iy >= (unsigned)p.H || (unsigned)ix >= (unsigned)p.W) continue;
            const float* px = in + ((size_t)iy * p.W + ix) * p.in_cs;
            for (int c = 0; c < p.cin_valid; ++c)
                acc = fmaf(px[c], wg[(((size_t)tap * (p.cin_pad >> 2) + (c >> 2)) * p.cout_pad + co) * 4 + (c & 3)], acc);
        }
        float v = fmaf(acc, p.scale[g * p.cout_pad + co], p.shift[g * p.cout_pad + co]);
        const size_t pix = ((size_t)b * p.Ho + oy) * p.Wo + ox;
        if (p.res) v += p.res[pix * p.res_cs + p.res_co + g * p.res_gs + co];
        if (p.relu && co >= p.relu_from) v = fmaxf(v, 0.f);
        p.out[(size_t)b * p.out_bs + (size_t)oy * p.out_rs + (size_t)ox * p.out_cs + p.out_co + g * p.out_gs + co] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// dispatch
// ------------------------------------------------------------------------------------------------
// The bf16x3 family (conv_bx3.hip: 26 instantiations, a minute of compile time) is an OPTIONAL part of the library since round 6: no
// committed variant table selects it (f16x2 is faster and as accurate), `--conv_math bf16x3` remains a tested arithmetic mode of a
// build made with ROMP_WITH_BX3=1 (romp_amd/build.py).  Without conv_bx3.o this weak definition answers: no variants.
__attribute__((weak)) ConvVariant* conv_variants_bx3(int* n) { *n = 0; return nullptr; }

static std::vector<ConvVariant> kVariants;
static int kNumVariants = 0;
static void collect_variants() {
    static const bool once = [] {
        int n = 0;
        ConvVariant* t = conv_variants_f32(&n); kVariants.insert(kVariants.end(), t, t + n);
        t = conv_variants_bx3(&n); if (n) kVariants.insert(kVariants.end(), t, t + n);
        t = conv_variants_h2(&n); kVariants.insert(kVariants.end(), t, t + n);
        t = conv_variants_h2d(&n); kVariants.insert(kVariants.end(), t, t + n);
        t = conv_variants_h2r(&n); kVariants.insert(kVariants.end(), t, t + n);
        t = conv_variants_h2s(&n); kVariants.insert(kVariants.end(), t, t + n);
        t = conv_variants_h2k(&n); kVariants.insert(kVariants.end(), t, t + n);
        t = conv_variants_h2g(&n); kVariants.insert(kVariants.end(), t, t + n);      // (appended last: the indices of older variants do not move)
        kNumVariants = (int)kVariants.size();
        return true;
    }();
    (void)once;
}

static const int kMaxLds = 160 * 1024;

// this unit's part of device_init: LDS limits and occupancies of the generic conv variants
static int setup_conv_variants() {
    collect_variants();
    for (int i = 0; i < kNumVariants; ++i) {
        if (kVariants[i].lds > kMaxLds) continue;
        if (kVariants[i].lds > 48 * 1024)
            ROMP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kVariants[i].fn),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, kVariants[i].lds));
        int occ = 0;
        ROMP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void*>(kVariants[i].fn),
                                                                    kVariants[i].threads ? kVariants[i].threads : (kVariants[i].pp ? 512 : 256), kVariants[i].lds));
        kVariants[i].occ = occ > 0 ? occ : 1;
    }
    return ROMP_OK;
}

static DeviceInfo g_dev;
const DeviceInfo& device() { return g_dev; }

// One device per process (the design: one process per GPU, torch.distributed over RCCL): limits, CU count, zero page and occupancies
// are kept per PROCESS.  A net on another device would silently run with the first device's, so it is refused.  A pointer
// that a failed attempt allocated is kept for the retry.
int device_init() {
    static std::mutex mu;
    static int device = -1;                 // >= 0: set up, for that device
    std::lock_guard<std::mutex> lock(mu);
    int dev = -1;
    ROMP_HIP_CHECK(hipGetDevice(&dev));
    ROMP_REQUIRE(device < 0 || dev == device, "this process already runs nets on device %d; libromp_hip.so serves ONE device per "
                 "process (launch one process per GPU), current device is %d", device, dev);
    if (device >= 0) return ROMP_OK;
    hipDeviceProp_t prop;
    ROMP_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    g_dev.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (!g_dev.queue_scratch) ROMP_HIP_CHECK(hipMalloc((void**)&g_dev.queue_scratch, QUEUE_INTS * sizeof(int)));
    if (!g_dev.zero) ROMP_HIP_CHECK(hipMalloc((void**)&g_dev.zero, 256));
    ROMP_HIP_CHECK(hipMemset(g_dev.zero, 0, 256));
    { const char* e = getenv("ROMP_CONV_TRACE");
      if (e && atoi(e) && !g_dev.trace) ROMP_HIP_CHECK(hipMalloc((void**)&g_dev.trace, (size_t)TRACE_WAVES * TRACE_SLOTS * sizeof(unsigned long long))); }
    int (*const units[])() = {setup_conv_variants, setup_bblock32, setup_bblock32r, setup_bblock64, setup_seam1x1, setup_fuseup, setup_stem2, setup_stem7p};
    for (auto unit : units) {
        const int rc = unit();
        if (rc) return rc;
    }
    device = dev;
    return ROMP_OK;
}

static bool variant_ok(const ConvVariant& v, const romp_op& op, int Ho, int Wo) {
    if (v.lds > kMaxLds) return false;
    if ((v.math == MATH_BX3 || v.math == MATH_BXD) && (op.weight_aux == nullptr || (op.cin_pad & 15))) return false;
    if (v.math >= MATH_H2 && (op.weight_h2 == nullptr || op.scale_h2 == nullptr || (op.cin_pad & 15))) return false;
    if (op.in_fmt == ROMP_FMT_H2 && v.math < MATH_H2) return false;
    if (v.math == MATH_H2K && !(op.out_fmt == ROMP_FMT_H2 && op.Cout == op.cout_pad && (op.res_buf == ROMP_BUF_NONE || op.res_fmt == ROMP_FMT_H2) &&
                          op.out_rstride == 0 && op.out_bstride == 0)) return false;      // conv_h2k: the direct H2 epilogue is its only one
    if (v.math >= MATH_H2R && op.in_fmt != ROMP_FMT_H2) return false;                         // register-weight kernels: pixels arrive by LDS-DMA too   // the DMA pipeline copies pre-split pixels
    if ((op.out_fmt == ROMP_FMT_H2 || op.res_fmt == ROMP_FMT_H2) && !(op.Cout == op.cout_pad)) return false;   // vector epilogue only
    if (v.ks != op.ksize || v.s != op.stride) return false;
    if (Wo % v.tw) return false;                     // rows may be partial (masked), columns may not
    if (op.cin_pad % v.ck || op.cout_pad % (v.nt * 32)) return false;
    return true;
}

// Heuristic choice (used until romp_net_autotune has measured the alternatives).
static int choose_variant(const romp_op& op, int Ho, int Wo, int B) {
    int best = -1;
    double best_score = -1;
    for (int i = 0; i < kNumVariants; ++i) {
        const ConvVariant& v = kVariants[i];
        if (!variant_ok(v, op, Ho, Wo)) continue;
        if (v.math && op.in_fmt != ROMP_FMT_H2) continue;       // split-precision variants are chosen by autotune / explicitly (H2 input: they are the only ones)
        const long items = (long)B * ((Ho + v.th - 1) / v.th) * (Wo / v.tw) * (op.cout_pad / (v.nt * 32)) * op.groups;
        const double eff = (double)Ho / (((Ho + v.th - 1) / v.th) * v.th);   // partial row tiles waste MFMA work
        double fill = items >= 512 ? 1.0 : (double)items / 512.0;
        double score = eff * fill * (1.0 + 0.25 * (v.mt * v.nt - 1)) * (v.ck >= 16 ? 1.0 : 0.8) * (v.tw == 32 ? 1.05 : 1.0);
        if (v.mt * v.nt > 4) score *= 0.5;
        if (score > best_score) { best_score = score; best = i; }
    }
    return best;
}

void conv_out_dims(const romp_op& op, int* Ho, int* Wo) {
    const int kh = op.ksize == 13 ? 1 : op.ksize, kw = op.ksize == 13 ? 3 : op.ksize;
    if (op.ksize == 2) { *Ho = op.H / op.stride; *Wo = op.W / op.stride; return; }   // 2x2: pad_h + (the other side) = 1 in total
    *Ho = (op.H + 2 * (kh / 2) - kh) / op.stride + 1;
    *Wo = (op.W + 2 * (kw / 2) - kw) / op.stride + 1;
}

int conv_num_variants() { collect_variants(); return kNumVariants; }
int conv_family_variants(int math) {
    collect_variants();
    int c = 0;
    for (const ConvVariant& v : kVariants) c += v.math == math;
    return c;
}

bool conv_variant_valid(const romp_op& op, int variant);
bool conv_variant_tunable(const romp_op& op, int variant) { return conv_variant_valid(op, variant); }

bool conv_variant_valid(const romp_op& op, int variant) {
    collect_variants();
    int Ho, Wo;
    conv_out_dims(op, &Ho, &Wo);
    return variant >= 0 && variant < kNumVariants && variant_ok(kVariants[variant], op, Ho, Wo);
}

int launch_conv(const romp_op& op, const float* in, const float* res, float* out, int B, int mode,
                int variant, int* queue, const LaunchCtx& c) {
    const hipStream_t st = c.st;
    ROMP_REQUIRE(op.ksize == 1 || op.ksize == 2 || op.ksize == 3 || op.ksize == 13, "conv: ksize %d unsupported", op.ksize);
    ROMP_REQUIRE(op.stride == 1 || op.stride == 2, "conv: stride %d unsupported", op.stride);
    ROMP_REQUIRE(op.groups >= 1, "conv: groups must be >= 1");
    ROMP_REQUIRE((op.in_cstride & 3) == 0 && (op.in_coff & 3) == 0 && (op.in_gstride & 3) == 0 && (op.Cin & 3) == 0,
                 "conv: input channels must be float4 aligned (cs %d co %d Cin %d)", op.in_cstride, op.in_coff, op.Cin);
    ConvParams p;
    p.in = in; p.w = op.weight; p.scale = op.scale; p.shift = op.shift; p.res = res; p.out = out;
    p.w3 = reinterpret_cast<const uint4*>(op.weight_aux);
    p.wh = reinterpret_cast<const uint4*>(op.weight_h2);
    p.scale_h = op.scale_h2;
    p.zero = g_dev.zero;
    p.act_scale = ldexpf(1.f, op.act_shift);
    p.inv_act_scale = ldexpf(1.f, -op.act_shift);
    p.in_h2 = op.in_fmt == ROMP_FMT_H2; p.out_h2 = op.out_fmt == ROMP_FMT_H2; p.res_h2 = res && op.res_fmt == ROMP_FMT_H2;
    if (p.in_h2 || p.out_h2 || p.res_h2) {
        ROMP_REQUIRE(mode == 0, "conv: the naive cross-check kernel only handles float32 tensors");
        ROMP_REQUIRE(((op.in_cstride | op.in_coff | op.in_gstride) & 7) == 0 || !p.in_h2, "conv: H2 input needs octet-aligned channels");
        ROMP_REQUIRE(((op.out_cstride | op.out_coff | op.out_gstride | op.Cout) & 7) == 0 || !p.out_h2, "conv: H2 output needs octet-aligned channels");
        ROMP_REQUIRE(((op.res_cstride | op.res_coff | op.res_gstride) & 7) == 0 || !p.res_h2, "conv: H2 residual needs octet-aligned channels");
    }
    p.H = op.H; p.W = op.W;
    conv_out_dims(op, &p.Ho, &p.Wo);
    p.Cout = op.Cout; p.cin_valid = op.Cin; p.cin_pad = op.cin_pad; p.cout_pad = op.cout_pad;
    p.in_cs = op.in_cstride; p.in_co = op.in_coff; p.in_gs = op.in_gstride;
    p.out_cs = op.out_cstride; p.out_co = op.out_coff; p.out_gs = op.out_gstride;
    p.res_cs = op.res_cstride; p.res_co = op.res_coff; p.res_gs = op.res_gstride;
    p.relu = op.relu;
    p.relu_from = op.relu ? op.relu_from : 0;
    ROMP_REQUIRE(p.relu_from >= 0 && (p.relu_from & 31) == 0, "conv: relu_from %d must be a multiple of 32", op.relu_from);
    p.sat = c.sat;
    p.w_gs = (op.ksize == 13 ? 3 : op.ksize * op.ksize) * op.cin_pad * op.cout_pad;
    const int kh = op.ksize == 13 ? 1 : op.ksize, kw = op.ksize == 13 ? 3 : op.ksize;
    p.pad_h = op.pad_h >= 0 ? op.pad_h : kh / 2;
    p.pad_w = op.pad_w >= 0 ? op.pad_w : kw / 2;
    p.out_rs = op.out_rstride > 0 ? op.out_rstride : p.Wo * op.out_cstride;
    p.out_bs = op.out_bstride > 0 ? op.out_bstride : p.Ho * p.Wo * op.out_cstride;
    p.tiles_x = p.tiles_y = p.tiles_total = 1;
    p.nslices = p.ns_total = p.n_queues = p.per_queue = 1;
    p.queue = nullptr;
    p.trace = nullptr;
    p.vec_io = (op.Cout == op.cout_pad && (op.Cout & 3) == 0 && (op.out_cstride & 3) == 0 && (op.out_coff & 3) == 0 && (op.out_gstride & 3) == 0 &&
                (!res || ((op.res_cstride & 3) == 0 && (op.res_coff & 3) == 0 && (op.res_gstride & 3) == 0))) ? 1 : 0;
    ROMP_REQUIRE(p.vec_io || !(p.out_h2 || p.res_h2), "conv: H2 output / residual needs the vector epilogue (Cout %d, pad %d)", op.Cout, op.cout_pad);
    if (mode == 1) {
        const size_t total = (size_t)B * p.Ho * p.Wo * op.Cout * op.groups;
        int blocks = (int)((total + 255) / 256);
        if (blocks > 65535) blocks = 65535;
        hipLaunchKernelGGL(conv_naive_kernel, dim3(blocks), dim3(256), 0, st, p, op.ksize, op.stride, B, op.groups);
        ROMP_HIP_CHECK(hipGetLastError());
        return ROMP_OK;
    }
    if (variant < 0) variant = choose_variant(op, p.Ho, p.Wo, B);
    ROMP_REQUIRE(variant >= 0 && variant < kNumVariants && variant_ok(kVariants[variant], op, p.Ho, p.Wo),
                 "conv: no kernel variant (%d) for k%d s%d Cin %d(pad %d) Cout %d(pad %d) out %dx%d", variant,
                 op.ksize, op.stride, op.Cin, op.cin_pad, op.Cout, op.cout_pad, p.Ho, p.Wo);
    const ConvVariant& v = kVariants[variant];
    p.tiles_x = p.Wo / v.tw;
    p.tiles_y = (p.Ho + v.th - 1) / v.th;
    p.tiles_total = B * p.tiles_x * p.tiles_y;
    p.nslices = op.cout_pad / (v.nt * 32);
    p.ns_total = p.nslices * op.groups;
    p.n_queues = (p.tiles_total % 8 == 0) ? 8 : 1;
    p.per_queue = (p.tiles_total / p.n_queues) * p.ns_total;
    if (queue == nullptr) {
        queue = g_dev.queue_scratch;
        ROMP_HIP_CHECK(hipMemsetAsync(queue, 0, QUEUE_INTS * sizeof(int), st));
    }
    p.queue = queue;
    const long items = (long)p.tiles_total * p.ns_total;
    long grid = (long)g_dev.num_cu * ((c.wg_cap > 0 && c.wg_cap < v.occ) ? c.wg_cap : v.occ);   // wg_cap: leave room for a co-resident kernel
    const long want = v.pp ? (items + 1) / 2 : items;         // a ping-pong workgroup runs two item streams
    if (grid > want) grid = want;
    if (p.n_queues == 8) grid = grid >= 8 ? (grid / 8) * 8 : 8;    // same number of workgroups per queue
    if (g_dev.trace) {
        p.trace = g_dev.trace;
        ROMP_HIP_CHECK(hipMemsetAsync(g_dev.trace, 0, (size_t)TRACE_WAVES * TRACE_SLOTS * sizeof(unsigned long long), st));
    }
    hipLaunchKernelGGL(v.fn, dim3((unsigned)grid), dim3(v.threads ? v.threads : (v.pp ? 512 : 256)), v.lds, st, p);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

// the (zeroed) stamp buffer for a kernel launched outside launch_conv (the fused BasicBlock), or nullptr when tracing is off
unsigned long long* conv_trace_arm(hipStream_t st) {
    if (!g_dev.trace) return nullptr;
    {   // never memset inside a stream capture (the fused kernels call this from their launch path): tracing is a debugging aid for
        // eager launches (romp_net_profile, romp_conv_forward)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return nullptr;
    }
    if (hipMemsetAsync(g_dev.trace, 0, (size_t)TRACE_WAVES * TRACE_SLOTS * sizeof(unsigned long long), st) != hipSuccess) return nullptr;
    return g_dev.trace;
}

int conv_trace_read(unsigned long long* dst_host, int max_words) {
    ROMP_REQUIRE(g_dev.trace != nullptr, "conv trace is off (set ROMP_CONV_TRACE=1 before the first launch)");
    const int n = max_words < TRACE_WAVES * TRACE_SLOTS ? max_words : TRACE_WAVES * TRACE_SLOTS;
    ROMP_HIP_CHECK(hipDeviceSynchronize());
    ROMP_HIP_CHECK(hipMemcpy(dst_host, g_dev.trace, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return n;
}

// family -> the name tune tables and profiles/ key on; `alt`: its ping-pong (f32) / four-workgroups-per-CU (f16x2) build
static const struct { ConvMath math; const char* name; const char* alt; } kFamilies[] = {
    {MATH_F32, "conv_mfma", "conv_pp"}, {MATH_BX3, "conv_bx3", "conv_bx3"}, {MATH_BXD, "conv_bxd", "conv_bxd"},
    {MATH_H2, "conv_h2", "conv_h2o"},   {MATH_H2D, "conv_h2d", "conv_h2do"}, {MATH_H2R, "conv_h2r", "conv_h2r"},
    {MATH_H2S, "conv_h2s", "conv_h2s"}, {MATH_H2K, "conv_h2k", "conv_h2k"},  {MATH_H2G, "conv_h2g", "conv_h2g"},
};

int describe_conv(const romp_op& op, int B, int variant, char* out, int n) {
    collect_variants();
    int Ho, Wo;
    conv_out_dims(op, &Ho, &Wo);
    if (variant < 0) variant = choose_variant(op, Ho, Wo, B);
    ROMP_REQUIRE(variant >= 0 && variant < kNumVariants, "describe: no variant");
    const ConvVariant& v = kVariants[variant];
    const char* name = "conv";
    for (const auto& f : kFamilies)
        if (f.math == v.math) name = (v.pp || v.o4) ? f.alt : f.name;
    snprintf(out, n, "%s_k%ds%d_mt%d_nt%d_tw%d_ck%d", name, v.ks, v.s, v.mt, v.nt, v.tw, v.ck);
    return ROMP_OK;
}

}  // namespace romp
