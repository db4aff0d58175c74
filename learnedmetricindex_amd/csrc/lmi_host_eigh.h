// lmi_host_eigh.h -- lmi_eigh: argument checks, the plan (lmi_eigh_plan.h), the call's device buffers, and the schedule on the NULL
// stream of the device: max|a| over the upper triangle and the finite check, then either the one launch of the resident form or, per
// sweep, the D - 1 round launches of the streamed form and one read of the sweep's "any pair rotated" word, then the order of the
// eigenvalues and the output rows.  Nothing of the caller's is written before the solve has converged.  lmi_eigh_set_geometry,
// lmi_debug_eigh_plan.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_eigh.h"
#include "lmi_eigh_plan.h"
#include <cmath>
#include <cstring>

static_assert(LMI_EIGH_SWEEP_CAP == lmi_eigh_plan::SWEEP_CAP && LMI_EIGH_MAX_D == lmi_eigh_plan::MAX_D, "one cap, one bound: header and plan");
static_assert(LMI_EIGH_FORM_RESIDENT == lmi_eigh_plan::FORM_RESIDENT && LMI_EIGH_FORM_STREAMED == lmi_eigh_plan::FORM_STREAMED, "the forms");

namespace {

thread_local lmi_eigh_plan::Forced g_eigh_forced;
thread_local int64_t g_eigh_last[LMI_EIGH_PLAN_COUNT] = {};

int eigh_round_launch(const lmi_eigh_plan::Plan& p, const double* Ain, double* Aout, const double* Vin, double* Vout, int r, int* rotated) {
    if (p.tile == lmi_eigh_plan::TILE_SMALL)
        eigh_round_kernel<lmi_eigh_plan::TILE_SMALL><<<p.grid, lmi_eigh_plan::TILE_SMALL * lmi_eigh_plan::TILE_SMALL>>>(
            Ain, Aout, Vin, Vout, p.d, r, p.tiles_side, p.a_tiles, rotated);
    else
        eigh_round_kernel<lmi_eigh_plan::TILE_LARGE><<<p.grid, lmi_eigh_plan::TILE_LARGE * lmi_eigh_plan::TILE_LARGE>>>(
            Ain, Aout, Vin, Vout, p.d, r, p.tiles_side, p.a_tiles, rotated);
    return 0;
}

int eigh_run(int device, const double* a, int d, int m, double* w, double* v, int* sweeps_out, int on_device) {
    const char* who = "lmi_eigh";
    for (int64_t& x : g_eigh_last) x = 0;
    if (!a || !w || !v) return fail("%s: a, w and v must not be NULL", who);
    if (d < 1 || d > lmi_eigh_plan::MAX_D) return fail("%s: d %d outside [1,%d]", who, d, lmi_eigh_plan::MAX_D);
    if (m < 1 || m > d) return fail("%s: m %d outside [1, d = %d]", who, m, d);
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));
    const lmi_eigh_plan::Plan p = lmi_eigh_plan::make_plan(d, g_eigh_forced);
    if (!p.form) return fail("%s: the resident form holds d <= %d, not d = %d", who, lmi_eigh_plan::RESIDENT_MAX_D, d);

    const size_t dd = (size_t)d * d * 8;
    CallScratch mem(who);
    double *d_a = const_cast<double*>(a), *d_w = w, *d_v = v;
    if (!on_device) {
        CHK(mem.alloc(&d_a, dd, "a"));
        CHK(upload_pieces(d_a, a, dd));
    }
    // max|a_ij|, i <= j, and the non-finite check
    unsigned long long* d_max = nullptr;
    unsigned long long h_max = 0;
    CHK(mem.alloc(&d_max, 8, "max"));
    HIPCHK(hipMemsetAsync(d_max, 0, 8, nullptr));
    eigh_absmax_kernel<<<(int)std::min<long long>(prop.multiProcessorCount * 8, cdiv((long long)d * d, 256)), 256>>>(d_a, d, d_max);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&h_max, d_max, 8, hipMemcpyDeviceToHost));
    if (h_max >= 0x7ff0000000000000ull) return fail("%s: the upper triangle of a holds a value that is not finite (inf or NaN)", who);
    int e = 0;   // the smallest integer with max|a_ij| < 2^e (0 for the zero matrix)
    if (h_max) {
        double mx;
        std::memcpy(&mx, &h_max, 8);
        (void)std::frexp(mx, &e);
    }

    const double* diag = nullptr;   // the eigenvalues of A = a 2^(-e), unordered, `stride` doubles apart
    long long stride = 1;
    const double* V = nullptr;
    int sweeps = 0, launches = 0;
    bool converged = false;
    if (p.form == lmi_eigh_plan::FORM_RESIDENT) {
        double *d_diag = nullptr, *d_V = nullptr;
        int* d_status = nullptr;
        int h_status[2] = {0, 0};
        CHK(mem.alloc(&d_diag, (size_t)d * 8, "eigenvalues"));
        CHK(mem.alloc(&d_V, dd, "V"));
        CHK(mem.alloc(&d_status, 8, "status"));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&eigh_resident_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)p.lds_bytes));
        eigh_resident_kernel<<<1, lmi_eigh_plan::RESIDENT_THREADS, (size_t)p.lds_bytes>>>(d_a, d, e, d_diag, d_V, d_status);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(h_status, d_status, 8, hipMemcpyDeviceToHost));
        sweeps = h_status[0];
        converged = h_status[1] != 0;
        launches = 1;
        diag = d_diag;
        V = d_V;
    } else {
        double *A2[2] = {nullptr, nullptr}, *V2[2] = {nullptr, nullptr};
        int* d_rot = nullptr;   // one "any pair rotated" word per sweep
        for (int b = 0; b < 2; ++b) {
            CHK(mem.alloc(&A2[b], dd, "A"));
            CHK(mem.alloc(&V2[b], dd, "V"));
        }
        CHK(mem.alloc(&d_rot, lmi_eigh_plan::SWEEP_CAP * 4, "rotated words"));
        HIPCHK(hipMemsetAsync(d_rot, 0, lmi_eigh_plan::SWEEP_CAP * 4, nullptr));
        eigh_init_kernel<<<cdiv((long long)d * d, 256), 256>>>(d_a, d, e, A2[0], V2[0]);
        HIPCHK(hipGetLastError());
        int cur = 0;
        while (sweeps < lmi_eigh_plan::SWEEP_CAP && !converged) {
            for (int r = 0; r < p.D - 1; ++r, cur ^= 1) CHK(eigh_round_launch(p, A2[cur], A2[cur ^ 1], V2[cur], V2[cur ^ 1], r, d_rot + sweeps));
            HIPCHK(hipGetLastError());
            launches += p.D - 1;
            int h_rot = 0;
            HIPCHK(hipMemcpy(&h_rot, d_rot + sweeps, 4, hipMemcpyDeviceToHost));   // once per sweep, not per round
            ++sweeps;
            converged = h_rot == 0;
        }
        diag = A2[cur];
        stride = (long long)d + 1;
        V = V2[cur];
    }
    if (!converged) return fail("%s: no convergence within %d sweeps", who, lmi_eigh_plan::SWEEP_CAP);

    int* d_order = nullptr;
    CHK(mem.alloc(&d_order, (size_t)d * 4, "order"));
    if (!on_device) {
        CHK(mem.alloc(&d_w, (size_t)m * 8, "w"));
        CHK(mem.alloc(&d_v, (size_t)m * d * 8, "v"));
    }
    HIPCHK(hipMemsetAsync(d_order, 0, (size_t)d * 4, nullptr));
    eigh_order_kernel<<<cdiv(d, 256), 256>>>(diag, stride, d, d_order);
    eigh_output_kernel<<<m, 256>>>(diag, stride, V, d_order, d, e, d_w, d_v);
    HIPCHK(hipGetLastError());
    if (!on_device) {
        HIPCHK(hipMemcpy(w, d_w, (size_t)m * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(v, d_v, (size_t)m * d * 8, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipStreamSynchronize(nullptr));
    if (sweeps_out) *sweeps_out = sweeps;
    g_eigh_last[LMI_EIGH_PLAN_FORM] = p.form;
    g_eigh_last[LMI_EIGH_PLAN_TILE] = p.tile;
    g_eigh_last[LMI_EIGH_PLAN_LDS_BYTES] = p.lds_bytes;
    g_eigh_last[LMI_EIGH_PLAN_RESIDENT_MAX_D] = lmi_eigh_plan::RESIDENT_MAX_D;
    g_eigh_last[LMI_EIGH_PLAN_GRID] = p.grid;
    g_eigh_last[LMI_EIGH_PLAN_SWEEPS] = sweeps;
    g_eigh_last[LMI_EIGH_PLAN_LAUNCHES] = launches;
    g_eigh_last[LMI_EIGH_PLAN_EXPONENT] = e;
    g_eigh_last[LMI_EIGH_PLAN_WORKSPACE_BYTES] = mem.total;
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_eigh_set_geometry(int form, int tile) {
    if (form != 0 && form != lmi_eigh_plan::FORM_RESIDENT && form != lmi_eigh_plan::FORM_STREAMED)
        return fail("lmi_eigh_set_geometry: form %d is none of 0, %d (resident), %d (streamed)", form, lmi_eigh_plan::FORM_RESIDENT,
                    lmi_eigh_plan::FORM_STREAMED);
    if (tile != 0 && tile != lmi_eigh_plan::TILE_SMALL && tile != lmi_eigh_plan::TILE_LARGE)
        return fail("lmi_eigh_set_geometry: tile %d is none of 0, %d, %d", tile, lmi_eigh_plan::TILE_SMALL, lmi_eigh_plan::TILE_LARGE);
    g_eigh_forced.form = form;
    g_eigh_forced.tile = tile;
    return 0;
}

extern "C" LMI_API int lmi_debug_eigh_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_eigh_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_EIGH_PLAN_COUNT); ++i) out[i] = g_eigh_last[i];
    return 0;
}

extern "C" LMI_API int lmi_eigh(int device, const double* a, int d, int m, double* w, double* v, int* sweeps, int on_device) {
    return eigh_run(device, a, d, m, w, v, sweeps, on_device);
}
