// lmi_host.h -- what every host-side header shares: the kernel headers, the handle (lmi_handle.h) and the
// per-call helpers (timing events and device stamps, input staging, the library's side stream).
#pragma once
#include "lmi_kernels.h"
#include "lmi_prefilter.h"
#include "lmi_pass2.h"
#include "lmi_pass2_small.h"
#include "lmi_mlp_fused.h"
#include "lmi_rescore.h"
#include "lmi_front.h"
#include "lmi_tail.h"
#include "lmi_mutate.h"
#include "lmi_store16.h"

#include "lmi_handle.h"   // error reporting, DevBuf, the handle and its parts, clone_handle
#include "lmi_layout.h"   // the bucket layout's arithmetic (host only, pure)

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <initializer_list>

#include "lmi_hip.h"

using namespace lmi;

static_assert(LMI_STORAGE_F32 == 0 && LMI_METRIC_IP == 0, "lmi_handle.h spells the defaults of storage / storage_req / metric as 0");
static_assert(lmi_layout::TILE_ROWS == P2_TILE_ROWS, "lmi_layout.h spells pass 2's tile rows as a number");

namespace {
inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
inline long long rup(long long a, long long b) { return (a + b - 1) / b * b; }
}  // namespace

// the low-dimensional form of the prefilter (d <= 128: lmi_pass2_small.h) for an index of kg16 k16-groups; otherwise pass2_kernel
static bool low_d_form(const lmi_index* h, int kg16) { return h->pf_small && kg16 <= PS_MAXKG; }
// which fp16 fragment shape the index and the queries are packed in: 16 x 32 for pass2_kernel, 32 x 16 for the low-dimensional kernels
static int frag16x16(const lmi_index* h) { return low_d_form(h, h->KG16) ? 0 : 1; }

// ---- the stored images: which form of the vectors a handle keeps, and every per-row image of that form ----
enum StoredForm {
    FORM_FRAG32,    // f32 fragments (`slab`): lmi_set_prefilter(0), the all-f32 scan
    FORM_ROWMAJOR,  // row-major f32 (`rowmajor`: exact re-rank / fallback / read-back) + the fp16 fragments (`slab16`) lmi_buckets_end derives
    FORM_FRAG16,    // fp16 fragments only (`slab16`): LMI_STORAGE_F16 (lmi_store16.h)
};
static StoredForm stored_form(const lmi_index* h) {
    return h->storage == LMI_STORAGE_F16 ? FORM_FRAG16 : h->prefilter ? FORM_ROWMAJOR : FORM_FRAG32;
}
// behind the fp16 fragments: pass2_kernel's look-ahead requests up to two stages = 4 KiB past the last row-block's fragments before it
// learns that the item is over; the data is never used, the addresses must be the allocation's
constexpr size_t P2_LOOKAHEAD_BYTES = 8192;
// One image: rb_bytes per row-block of the layout (+ extra behind the last); zeroed: lmi_buckets_begin zero-fills it (rows arrive
// piece by piece; the others are written whole before they are read).  An image of n row-blocks is allocated for at least one.
struct SlabImage {
    DevBuf* buf;
    size_t rb_bytes, extra;
    bool zeroed;
    size_t bytes(int64_t n_rb) const { return (size_t)std::max<int64_t>(n_rb, 1) * rb_bytes + extra; }
};
constexpr int MAX_SLAB_IMAGES = 3;
// every per-row image the handle keeps, row-block-major, the ids last.  planned: also the fp16 fragments that lmi_buckets_end has yet
// to derive (lmi_buckets_begin reserves them with the build's other images)
static int slab_images(lmi_index* h, SlabImage* im, bool planned = false) {
    int n = 0;
    switch (stored_form(h)) {
    case FORM_FRAG32: im[n++] = {&h->slab, (size_t)h->KGs * 1024, 0, true}; break;
    case FORM_ROWMAJOR:
        im[n++] = {&h->rowmajor, (size_t)32 * h->dp * 4, 0, true};
        if (h->have16 || planned) im[n++] = {&h->slab16, (size_t)h->KG16 * 1024, P2_LOOKAHEAD_BYTES, false};
        break;
    case FORM_FRAG16: im[n++] = {&h->slab16, (size_t)h->KG16 * 1024, P2_LOOKAHEAD_BYTES, true}; break;
    }
    im[n++] = {&h->ids_slab, 128, 0, false};
    return n;
}
static int64_t alloc_rb(lmi_index* h) {   // row-blocks every image's allocation holds
    SlabImage im[MAX_SLAB_IMAGES];
    const int n = slab_images(h, im);
    int64_t a = INT64_MAX;
    for (int i = 0; i < n; ++i) a = std::min<int64_t>(a, im[i].buf->cap < im[i].extra ? 0 : (int64_t)((im[i].buf->cap - im[i].extra) / im[i].rb_bytes));
    return a;
}

// why an LMI_STORAGE_F16 build cannot go with the handle's other settings (nullptr: it can)
static const char* storage16_conflict(const lmi_index* h) {
    if (!h->pf_hw_ok) return "the fp16 subnormal self-test failed on this device: the fp16 fragments cannot be trusted to hold the vectors";
    if (h->metric == LMI_METRIC_L2) return "LMI_METRIC_L2 is not supported (the -|x|^2/2 column of a stored vector is not fp16-exact)";
    if (!h->prefilter) return "lmi_set_prefilter(0) is not supported (the all-f32 scan needs f32 fragments)";
    return nullptr;
}

// the dynamic-LDS limits of the re-rank kernels' LMI_STORAGE_F16 forms: set when a handle first builds such an index (per device;
// handles that never do -- lmi_knn_ip's among them -- do not pay for it)
static int storage16_kernel_attrs(lmi_index* h) {
    if (h->attrs16_done) return 0;
#define LMI_RC16_ATTR(GV) \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rescore_kernel<GV, false, true, Frag16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rescore_kernel<GV, true, true, Frag16>), hipFuncAttributeMaxDynamicSharedMemorySize, RC_SMALL_LDS_CAP)); \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tail_kernel<GV, true, Frag16>), hipFuncAttributeMaxDynamicSharedMemorySize, RC_SMALL_LDS_CAP));
    LMI_RC16_ATTR(1) LMI_RC16_ATTR(2) LMI_RC16_ATTR(3) LMI_RC16_ATTR(4)
#undef LMI_RC16_ATTR
    h->attrs16_done = true;
    return 0;
}

static int set_dev(lmi_index* h) {
    HIPCHK(hipSetDevice(h->device));
    return 0;
}

// ---- per call: the timing ring, device stamps, input staging, the side stream ----
static void begin_call(lmi_index* h) {
    h->ev_cur = (h->ev_cur + 1) % lmi_index::EV_RING;
    h->ev = h->ev_ring[h->ev_cur];
    h->ev_valid = h->valid_ring[h->ev_cur];
    for (int i = 0; i < 10; ++i) h->ev_valid[i] = false;
    ++h->ev_calls;
    h->ts_mask[h->ev_cur] = 0u;
    h->ts_set = nullptr;
    if (h->timing_level == 2) {   // device stamps: the call's set of the ring (allocated with the first timed call; a failed allocation: no stamps)
        if (!h->ts_ring.p && h->ts_ring.reserve((size_t)lmi_index::EV_RING * ST_COUNT * 8) != 0) return;
        h->ts_set = h->ts_ring.as<unsigned long long>() + (size_t)h->ev_cur * ST_COUNT;
    }
}
// the device word a kernel of this call writes stamp `idx` to (nullptr: stamps are off)
static unsigned long long* tsp(lmi_index* h, int idx) {
    if (!h->ts_set) return nullptr;
    h->ts_mask[h->ev_cur] |= 1u << idx;
    return h->ts_set + idx;
}
// the end of a call whose last kernel carries no stamp (lmi_mlp_topk, lmi_nav_order ..): one single-thread launch behind it
static int stamp_end(lmi_index* h, int idx) {
    if (unsigned long long* p = tsp(h, idx)) {
        stamp_kernel<<<1, 1, 0, h->stream>>>(p);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

static int record(lmi_index* h, int i) {
    // every recorded event is a ~5 us bubble between two kernels: level 3 records every phase boundary, level 1 the call's first
    // and last event (LMI_T_TOTAL), levels 0 and 2 none (2: the kernels stamp the chip's clock themselves, tsp)
    if (h->timing_level == 0 || h->timing_level == 2 || (h->timing_level == 1 && i != 0 && i != 1 && i != 4)) return 0;
    if (!h->ev[i]) HIPCHK(hipEventCreateWithFlags(&h->ev[i], hipEventDisableSystemFence));   // timing only: no system-scope release at the record
    HIPCHK(hipEventRecord(h->ev[i], h->stream));
    h->ev_valid[i] = true;
    return 0;
}

// device pointer to the caller's input (uploads host data into `buf`)
static int input_ptr(lmi_index* h, const void* src, size_t bytes, int on_device, DevBuf& buf, const void** out) {
    if (on_device) { *out = src; return 0; }
    CHK(buf.reserve(bytes));
    HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    *out = buf.p;
    return 0;
}

// Binary16 sources (halves as uint16 bit patterns; a caller's pointer is only 2-byte aligned): a kernel may read 8 halves with one
// 16-byte load only where d % 8 == 0 and the base is 16-byte aligned -- then every row starts on a 16-byte boundary.  Per launch.
static bool half_src_vec(const void* src, int d) { return d % 8 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0; }
// n rows of d halves at `src` (device) -> binary32 at `dst` (a buffer of the library's: 16-byte aligned), on stream s
static int widen16_enqueue(const void* src, long long n, int d, float* dst, hipStream_t s) {
    const long long total = n * d;
    if (total == 0) return 0;
    if (half_src_vec(src, d)) widen16_kernel<true><<<cdiv(total >> 3, 256), 256, 0, s>>>(static_cast<const unsigned short*>(src), total, dst);
    else widen16_kernel<false><<<cdiv(total, 256), 256, 0, s>>>(static_cast<const unsigned short*>(src), total, dst);
    HIPCHK(hipGetLastError());
    return 0;
}
// device pointer to the binary32 form of a half input of n rows x d: the halves are uploaded (host data; half the bytes) into `raw` and
// widened into `buf`, the handle's buffer for that input; a device pointer is widened from where it lies (the caller's memory is only read)
static int input_ptr16(lmi_index* h, const void* src, long long n, int d, int on_device, DevBuf& raw, DevBuf& buf, const void** out) {
    CHK(buf.reserve((size_t)n * d * 4));
    if (!on_device) {
        CHK(raw.reserve((size_t)n * d * 2));
        HIPCHK(hipMemcpyAsync(raw.p, src, (size_t)n * d * 2, hipMemcpyHostToDevice, h->stream));
        src = raw.p;
    }
    else if (&buf == &h->q_srch) h->q_srch_async = true;
    CHK(widen16_enqueue(src, n, d, buf.as<float>(), h->stream));
    *out = buf.p;
    return 0;
}

// the end of a host-pointer call: the listed device arrays back to the caller's, on h->stream in the order given, then the
// synchronisation.  An entry whose host pointer is null is skipped: that is how optional outputs (keys, logits, the bucket order of
// a search) are declined, and a required output passed as null (never valid) is now skipped too, not handed to the copy
struct HostCopy { void* host; const void* dev; size_t bytes; };
static int copy_back(lmi_index* h, std::initializer_list<HostCopy> list) {
    for (const HostCopy& c : list)
        if (c.host) HIPCHK(hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// Side stream (library-owned): work that does not depend on what the handle's stream runs next is forked onto it and
// joined before its results are needed.  side_fork: the side stream waits for everything enqueued on h->stream so far.
static int side_ensure(lmi_index* h) {
    if (!h->side) {
        HIPCHK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&h->side_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->side_join, hipEventDisableTiming));
    }
    return 0;
}
static int side_fork(lmi_index* h) {
    CHK(side_ensure(h));
    HIPCHK(hipEventRecord(h->side_fork, h->stream));
    HIPCHK(hipStreamWaitEvent(h->side, h->side_fork, 0));
    return 0;
}
static int side_join(lmi_index* h) {
    HIPCHK(hipEventRecord(h->side_join, h->side));
    HIPCHK(hipStreamWaitEvent(h->stream, h->side_join, 0));
    return 0;
}
