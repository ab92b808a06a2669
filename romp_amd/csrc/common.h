// common.h -- shared helpers for libromp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/romp_hip.h"

namespace romp {

void set_error(const char* fmt, ...);

#define ROMP_HIP_CHECK(expr)                                                          \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            romp::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                            __FILE__, __LINE__);                                      \
            return ROMP_EHIP;                                                         \
        }                                                                             \
    } while (0)

#define ROMP_REQUIRE(cond, ...)                                                       \
    do {                                                                              \
        if (!(cond)) {                                                                \
            romp::set_error(__VA_ARGS__);                                             \
            return ROMP_EINVAL;                                                       \
        }                                                                             \
    } while (0)

// work queues of the persistent conv kernels: 8 counters (one per XCD), each on its own 128-byte line
constexpr int QUEUE_STRIDE = 32, QUEUE_INTS = 8 * QUEUE_STRIDE;

// What the executor tells a launch: the stream, the device counter its kernels report clamped values to (the net's; nullptr: nothing
// to report to) and the workgroups per CU a kernel may take (0: all it can; > 0: room for a co-resident kernel of another stream).
struct LaunchCtx { hipStream_t st; int* sat; int wg_cap; };

// Per-process device facts: device_init() (conv_mfma.hip) fills them once, every launcher reads them.
// zero: 256 bytes of zeros (out-of-image lanes of LDS-DMA pixel / halo fetches); queue_scratch: QUEUE_INTS ints for romp_conv_forward
// callers without an arena; trace: env ROMP_CONV_TRACE=1, per-wave phase stamps of the most recent split-precision launch
struct DeviceInfo { int num_cu = 256; float* zero = nullptr; int* queue_scratch = nullptr; unsigned long long* trace = nullptr; };
const DeviceInfo& device();
// Everything a launch needs that may not happen inside a stream capture: the record above, raised dynamic-LDS limits, occupancies.
// romp_net_create and romp_conv_forward call it (thread safe; a failure leaves romp_last_error() set and may be retried); no
// launcher does.  One device per process: a call with another current device than the first one's is refused.
int device_init();
// its per-unit parts: the kernels of one translation unit that need a raised dynamic-LDS limit (conv_h2b.hip, conv_h2c32.hip,
// conv_h2c.hip, conv_h2x.hip, conv_fup.hip, stem2.hip, stem7p.hip)
int setup_bblock32(), setup_bblock32r(), setup_bblock64(), setup_seam1x1(), setup_fuseup(), setup_stem2(), setup_stem7p();

// launchers implemented in the kernel translation units
// variant < 0: heuristic choice; queue: QUEUE_INTS zeroed ints (nullptr: library scratch, memset on the launch's stream)
int launch_conv(const romp_op& op, const float* in, const float* res, float* out, int B,
                int mode, int variant, int* queue, const LaunchCtx& c);
void conv_out_dims(const romp_op& op, int* Ho, int* Wo);         // output size of a ROMP_OP_CONV
int describe_conv(const romp_op& op, int B, int variant, char* out, int n);
int conv_num_variants();
int conv_family_variants(int math);                              // variants of one kernel family (ConvVariant.math) in this build
int conv_trace_read(unsigned long long* dst_host, int max_words);
bool conv_variant_valid(const romp_op& op, int variant);
bool conv_variant_tunable(const romp_op& op, int variant);   // ... and offered to romp_net_autotune
unsigned long long* conv_trace_arm(hipStream_t st);   // conv_mfma.hip: ROMP_CONV_TRACE stamp buffer, zeroed on `st` (nullptr: off)
// The fused launchers' (and the stem / pool / split-K tail launchers') requirements on the ops alone (shapes, formats, packs -- nothing
// that depends on B, on device pointers or on the device): romp_net_create runs them for every op of the kind BEFORE it touches the
// device (a host without one still gets the named refusal), the launcher runs them again in front of its B-dependent ones.
int check_seam1x1(const romp_op& opa, const romp_op& opb, const romp_op* opd);
int check_bblock32(const romp_op& op1, const romp_op& op2), check_bblock32r(const romp_op& op1, const romp_op& op2), check_bblock64(const romp_op& op1, const romp_op& op2);
int check_stem2(const romp_op& stem, const romp_op& op);
int check_stem7p(const romp_op& op);
int check_stem(const romp_op& op), check_stem7(const romp_op& op), check_maxpool(const romp_op& op), check_ksum(const romp_op& op);   // stem_fuse.hip
int check_fuseup(const romp_op& op);
int launch_seam1x1(const romp_op& opa, const romp_op& opb, const romp_op* opd, const float* m, const float* x, float* t, float* u, int B, const LaunchCtx& c);   // conv_h2x.hip
int launch_bblock32r(const romp_op& op1, const romp_op& op2, const float* x, float* y, int B, int* queue, const LaunchCtx& c);  // conv_h2c32.hip
int launch_bblock64(const romp_op& op1, const romp_op& op2, const float* x, float* y, int B, int* queue, const LaunchCtx& c);   // conv_h2c.hip
int launch_bblock32(const romp_op& op1, const romp_op& op2, const float* x, float* y, int B, int* queue, const LaunchCtx& c);
int launch_stem(const romp_op& op, const float* image, float* out, int B, const LaunchCtx& c);
int launch_stem7(const romp_op& op, const float* image, float* out, int B, const LaunchCtx& c);
int launch_stem2(const romp_op& stem, const romp_op& op, const float* image, float* out, int B, const LaunchCtx& c);   // stem2.hip
int launch_maxpool(const romp_op& op, const float* in, float* out, int B, const LaunchCtx& c);
int launch_stem7p(const romp_op& op, const float* image, float* out, int B, const LaunchCtx& c);   // stem7p.hip
struct FuseTerm { const float* ptr; int shift; int cstride; int fmt; };
int launch_fusesum(const FuseTerm* terms, int n_terms, float* out, int B, int H, int W, int C,
                   int out_cstride, int out_coff, int relu, const LaunchCtx& c, int out_fmt = 0, int act_shift = 0);

int launch_fuseup(const romp_op& op, const FuseTerm* terms, float* out, int B, const LaunchCtx& c);      // conv_fup.hip

int launch_ksum(const romp_op& op, const float* partial, const float* res, float* out, int B, const LaunchCtx& c);

// BEV head pieces (bev.hip); *_host pointers are dereferenced on the host at launch time
int launch_bev_pack(const float* fv, int fv_cs, const float* feats, int f_cs, float* out, int B, const LaunchCtx& c);
int launch_bev_maps(const float* fv, int fv_cs, const float* bv, int bv_cs, const float* anchors_host, float* center3d,
                    float* cam3d, int B, const LaunchCtx& c);
int launch_conv3d(int C, const float* w_host, const float* scale_host, const float* shift_host, int relu, const float* in,
                  const float* res, float* out, int B, const LaunchCtx& c);

}  // namespace romp
