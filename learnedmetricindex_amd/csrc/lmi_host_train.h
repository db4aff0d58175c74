// lmi_host_train.h -- lmi_train and lmi_train_f16 (one body over the type of x): argument checks, the call's device buffers, the gather of the named rows (on the host in pieces, or by
// a kernel), the finite check, and the step schedule (forward, softmax gradient, then per layer from the last: da, dW with Adam) on
// the NULL stream of the device.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_train.h"
#include <cmath>

namespace {

template <int MODE>
int tr_launch(const TrGemm& P) {
    tr_gemm_kernel<MODE><<<dim3(cdiv(P.N, 32), cdiv(P.M, 32)), 64>>>(P);
    HIPCHK(hipGetLastError());
    return 0;
}

// the named rows of a device array into the batch buffer, by the type of x
void tr_gather(int grid, const float* x, const int* labels, const long long* rows, long long nb, int d, int classes, float* xb, int* yb, int* bad) {
    tr_gather_kernel<<<grid, 256>>>(x, labels, rows, nb, d, classes, xb, yb, bad);
}
void tr_gather(int grid, const uint16_t* x, const int* labels, const long long* rows, long long nb, int d, int classes, float* xb, int* yb, int* bad) {
    tr_gather16_kernel<<<grid, 256>>>(x, labels, rows, nb, d, classes, xb, yb, bad);
}

template <class T>
int train_run(const char* who, int device, const T* x, int64_t n, const int32_t* labels, int n_layers, const int* dims, float* const* W,
              float* const* b, float* const* adam, int64_t* t, const int64_t* batch_rows, int n_steps, int bsz, double lr, float* losses,
              int on_device);

}  // namespace

extern "C" LMI_API int lmi_train(int device, const float* x, int64_t n, const int32_t* labels, int n_layers, const int* dims, float* const* W,
                                 float* const* b, float* const* adam, int64_t* t, const int64_t* batch_rows, int n_steps, int bsz, double lr,
                                 float* losses, int on_device) {
    return train_run<float>("lmi_train", device, x, n, labels, n_layers, dims, W, b, adam, t, batch_rows, n_steps, bsz, lr, losses, on_device);
}

extern "C" LMI_API int lmi_train_f16(int device, const uint16_t* x, int64_t n, const int32_t* labels, int n_layers, const int* dims,
                                     float* const* W, float* const* b, float* const* adam, int64_t* t, const int64_t* batch_rows, int n_steps,
                                     int bsz, double lr, float* losses, int on_device) {
    return train_run<uint16_t>("lmi_train_f16", device, x, n, labels, n_layers, dims, W, b, adam, t, batch_rows, n_steps, bsz, lr, losses,
                               on_device);
}

namespace {

template <class T>
int train_run(const char* who, int device, const T* x, int64_t n, const int32_t* labels, int n_layers, const int* dims, float* const* W,
              float* const* b, float* const* adam, int64_t* t, const int64_t* batch_rows, int n_steps, int bsz, double lr, float* losses,
              int on_device) {
    if (!x || !labels || !dims || !W || !b) return fail("%s: x, labels, dims, W and b must not be NULL", who);
    if (n < 1) return fail("%s: n %lld < 1", who, (long long)n);
    if (n_layers < 1 || n_layers > LMI_MAX_LAYERS) return fail("%s: n_layers %d outside [1,%d]", who, n_layers, LMI_MAX_LAYERS);
    for (int i = 0; i < n_layers; ++i)
        if (dims[i] < 1 || dims[i] > 4096) return fail("%s: dims[%d] = %d outside [1,4096]", who, i, dims[i]);
    const int d = dims[0], classes = dims[n_layers];
    if (classes < 1 || classes > 16384) return fail("%s: %d classes outside [1,16384]", who, classes);
    if (bsz < 1 || bsz > 256) return fail("%s: bsz %d outside [1,256]", who, bsz);
    if (n_steps < 0 || n_steps > 100000) return fail("%s: n_steps %d outside [0,100000]", who, n_steps);
    if (!std::isfinite(lr) || !(lr > 0.0)) return fail("%s: lr %g is not a finite positive number", who, lr);
    const int64_t t0 = t ? *t : 0;
    if (t0 < 0) return fail("%s: *t = %lld < 0", who, (long long)t0);
    for (int i = 0; i < n_layers; ++i)
        if (!W[i] || !b[i]) return fail("%s: NULL weight/bias for layer %d", who, i);
    if (adam)
        for (int i = 0; i < 4 * n_layers; ++i)
            if (!adam[i]) return fail("%s: adam[%d] is NULL", who, i);
    if (n_steps > 0 && !batch_rows) return fail("%s: batch_rows must not be NULL", who);
    const long long nb = (long long)n_steps * bsz;   // named rows
    for (long long j = 0; j < nb; ++j)
        if (batch_rows[j] < 0 || batch_rows[j] >= n)
            return fail("%s: batch_rows[%lld] = %lld outside [0,%lld)", who, j, (long long)batch_rows[j], (long long)n);
    if (!on_device)
        for (long long j = 0; j < nb; ++j) {
            const int lab = labels[batch_rows[j]];
            if (lab < 0 || lab >= classes) return fail("%s: the label %d of row %lld is outside [0,%d)", who, lab, (long long)batch_rows[j], classes);
        }
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));
    if (n_steps == 0) return 0;   // nothing to train on: the parameters, the moments and *t stay as they are

    CallScratch mem(who);
    float* d_xb = nullptr;
    int* d_yb = nullptr;
    CHK(mem.alloc(&d_xb, (size_t)nb * d * 4, "the named rows"));
    CHK(mem.alloc(&d_yb, (size_t)nb * 4, "their labels"));
    std::vector<float*> d_W(n_layers), d_b(n_layers), d_z(n_layers), d_g(n_layers);
    std::vector<float*> d_adam((size_t)4 * n_layers);
    for (int i = 0; i < n_layers; ++i) {
        const size_t wn = (size_t)dims[i + 1] * dims[i], bn = (size_t)dims[i + 1];
        CHK(mem.alloc(&d_W[i], wn * 4, "weights"));
        CHK(mem.alloc(&d_b[i], bn * 4, "biases"));
        CHK(mem.alloc(&d_z[i], (size_t)bsz * bn * 4, "layer outputs"));
        CHK(mem.alloc(&d_g[i], (size_t)bsz * bn * 4, "output gradients"));
        for (int q = 0; q < 4; ++q) CHK(mem.alloc(&d_adam[(size_t)4 * i + q], (q < 2 ? wn : bn) * 4, "Adam moments"));
    }
    float *d_lrow = nullptr, *d_loss = nullptr;
    unsigned* d_max = nullptr;   // [0]: max |x| of the named rows, [1]: of the initial weights and biases, [2]: a label out of range
    CHK(mem.alloc(&d_max, 12, "checks"));
    if (losses) {
        CHK(mem.alloc(&d_lrow, (size_t)bsz * 4, "row losses"));
        CHK(mem.alloc(&d_loss, (size_t)n_steps * 4, "losses"));
    }
    HIPCHK(hipMemsetAsync(d_max, 0, 12, nullptr));

    // the named rows and their labels, in batch_rows order
    const int gs = prop.multiProcessorCount * 8;
    if (on_device) {
        long long* d_rows = nullptr;
        CHK(mem.alloc(&d_rows, (size_t)nb * 8, "batch_rows"));
        HIPCHK(hipMemcpyAsync(d_rows, batch_rows, (size_t)nb * 8, hipMemcpyHostToDevice, nullptr));
        tr_gather((int)std::min<long long>(gs, cdiv(nb * d, 256)), x, labels, d_rows, nb, d, classes, d_xb, d_yb, reinterpret_cast<int*>(d_max + 2));
        HIPCHK(hipGetLastError());
    } else {
        // 64 MiB of rows at a time, in the type they came in: halves go up as halves into a piece buffer and are widened from there
        const long long piece_rows = std::max<long long>(1, ((long long)64 << 20) / ((long long)sizeof(T) * d));
        std::vector<T> stage((size_t)std::min(piece_rows, nb) * d);
        std::vector<int> yb((size_t)nb);
        uint16_t* d_x16 = nullptr;
        if constexpr (sizeof(T) == 2) CHK(mem.alloc(&d_x16, stage.size() * 2, "a piece of the named rows as halves"));
        for (long long j0 = 0; j0 < nb; j0 += piece_rows) {
            const long long m = std::min(piece_rows, nb - j0);
            for (long long j = 0; j < m; ++j) memcpy(&stage[(size_t)j * d], x + (size_t)batch_rows[j0 + j] * d, (size_t)d * sizeof(T));
            if constexpr (sizeof(T) == 2) {
                HIPCHK(hipMemcpy(d_x16, stage.data(), (size_t)m * d * 2, hipMemcpyHostToDevice));
                CHK(widen16_enqueue(d_x16, m, d, d_xb + (size_t)j0 * d, nullptr));
            } else {
                HIPCHK(hipMemcpy(d_xb + (size_t)j0 * d, stage.data(), (size_t)m * d * 4, hipMemcpyHostToDevice));
            }
        }
        for (long long j = 0; j < nb; ++j) yb[(size_t)j] = labels[batch_rows[j]];
        HIPCHK(hipMemcpy(d_yb, yb.data(), (size_t)nb * 4, hipMemcpyHostToDevice));
    }
    for (int i = 0; i < n_layers; ++i) {
        const size_t wn = (size_t)dims[i + 1] * dims[i], bn = (size_t)dims[i + 1];
        HIPCHK(hipMemcpyAsync(d_W[i], W[i], wn * 4, hipMemcpyHostToDevice, nullptr));
        HIPCHK(hipMemcpyAsync(d_b[i], b[i], bn * 4, hipMemcpyHostToDevice, nullptr));
        for (int q = 0; q < 4; ++q) {
            const size_t bytes = (q < 2 ? wn : bn) * 4;
            if (adam) HIPCHK(hipMemcpyAsync(d_adam[(size_t)4 * i + q], adam[4 * i + q], bytes, hipMemcpyHostToDevice, nullptr));
            else HIPCHK(hipMemsetAsync(d_adam[(size_t)4 * i + q], 0, bytes, nullptr));
        }
    }

    // the non-finite check of the named rows and of the initial weights, before the first step
    unsigned h_max[3] = {0, 0, 0};
    dense_absmax_kernel<<<(int)std::min<long long>(gs, cdiv(nb * d, 256)), 256>>>(d_xb, nb * d, d_max);
    for (int i = 0; i < n_layers; ++i) {
        const long long wn = (long long)dims[i + 1] * dims[i];
        dense_absmax_kernel<<<(int)std::min<long long>(gs, cdiv(wn, 256)), 256>>>(d_W[i], wn, d_max + 1);
        dense_absmax_kernel<<<cdiv(dims[i + 1], 256), 256>>>(d_b[i], dims[i + 1], d_max + 1);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(h_max, d_max, 12, hipMemcpyDeviceToHost));
    if (h_max[2]) return fail("%s: the label of a named row is outside [0,%d)", who, classes);
    if (h_max[0] >= 0x7f800000u) return fail("%s: a named row of x holds a value that is not finite (inf or NaN)", who);
    if (h_max[1] >= 0x7f800000u) return fail("%s: the initial weights hold a value that is not finite (inf or NaN)", who);

    // P1 = 0.9^t', P2 = 0.999^t' as running products in binary64 (once both are 0 they stay 0)
    double P1 = 1.0, P2 = 1.0;
    for (int64_t q = 0; q < t0 && (P1 != 0.0 || P2 != 0.0); ++q) { P1 *= 0.9; P2 *= 0.999; }
    const float inv_b = 1.0f / (float)bsz;
    for (int s = 0; s < n_steps; ++s) {
        P1 *= 0.9;
        P2 *= 0.999;
        const float step = (float)(lr / (1.0 - P1)), r2 = (float)std::sqrt(1.0 - P2);
        const float* xs = d_xb + (size_t)s * bsz * d;
        for (int i = 0; i < n_layers; ++i) {   // z_i = b_i + a_i . W_i^T
            TrGemm P{};
            P.A = i == 0 ? xs : d_z[i - 1]; P.a_sm = dims[i]; P.a_sk = 1; P.relu_a = i > 0;
            P.B = d_W[i]; P.b_sk = 1; P.b_sn = dims[i];
            P.M = bsz; P.N = dims[i + 1]; P.K = dims[i];
            P.bias = d_b[i]; P.out = d_z[i];
            CHK(tr_launch<TR_FWD>(P));
        }
        tr_softmax_grad_kernel<<<bsz, 64>>>(d_z[n_layers - 1], d_yb + (size_t)s * bsz, classes, inv_b, d_g[n_layers - 1], d_lrow);
        HIPCHK(hipGetLastError());
        for (int i = n_layers - 1; i >= 0; --i) {
            if (i > 0) {   // g_{i-1} = z_{i-1} > 0 ? g_i . W_i : +0, before W_i is touched
                TrGemm P{};
                P.A = d_g[i]; P.a_sm = dims[i + 1]; P.a_sk = 1;
                P.B = d_W[i]; P.b_sk = dims[i]; P.b_sn = 1;
                P.M = bsz; P.N = dims[i]; P.K = dims[i + 1];
                P.out = d_g[i - 1]; P.zprev = d_z[i - 1];
                CHK(tr_launch<TR_DA>(P));
            }
            TrGemm P{};   // dW_i = g_i^T . a_i, db_i, Adam
            P.A = d_g[i]; P.a_sm = 1; P.a_sk = dims[i + 1];
            P.B = i == 0 ? xs : d_z[i - 1]; P.b_sk = dims[i]; P.b_sn = 1; P.relu_b = i > 0;
            P.M = dims[i + 1]; P.N = dims[i]; P.K = bsz;
            P.W = d_W[i]; P.mW = d_adam[(size_t)4 * i]; P.vW = d_adam[(size_t)4 * i + 1];
            P.b = d_b[i]; P.mb = d_adam[(size_t)4 * i + 2]; P.vb = d_adam[(size_t)4 * i + 3];
            P.g = d_g[i];
            P.step = step; P.r2 = r2;
            if (losses && i == n_layers - 1) { P.lrow = d_lrow; P.loss = d_loss + s; }
            CHK(tr_launch<TR_DW>(P));
        }
    }
    // the outputs land in host copies first: a failed copy leaves the caller's arrays as they were
    std::vector<std::vector<float>> hW(n_layers), hb(n_layers), hadam(adam ? (size_t)4 * n_layers : 0);
    std::vector<float> hloss(losses ? (size_t)n_steps : 0);
    for (int i = 0; i < n_layers; ++i) {
        const size_t wn = (size_t)dims[i + 1] * dims[i], bn = (size_t)dims[i + 1];
        hW[i].resize(wn);
        hb[i].resize(bn);
        HIPCHK(hipMemcpy(hW[i].data(), d_W[i], wn * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hb[i].data(), d_b[i], bn * 4, hipMemcpyDeviceToHost));
        if (adam)
            for (int q = 0; q < 4; ++q) {
                auto& v = hadam[(size_t)4 * i + q];
                v.resize(q < 2 ? wn : bn);
                HIPCHK(hipMemcpy(v.data(), d_adam[(size_t)4 * i + q], v.size() * 4, hipMemcpyDeviceToHost));
            }
    }
    if (losses) HIPCHK(hipMemcpy(hloss.data(), d_loss, (size_t)n_steps * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(nullptr));
    for (int i = 0; i < n_layers; ++i) {
        memcpy(W[i], hW[i].data(), hW[i].size() * 4);
        memcpy(b[i], hb[i].data(), hb[i].size() * 4);
        if (adam)
            for (int q = 0; q < 4; ++q) memcpy(adam[4 * i + q], hadam[(size_t)4 * i + q].data(), hadam[(size_t)4 * i + q].size() * 4);
    }
    if (losses) memcpy(losses, hloss.data(), (size_t)n_steps * 4);
    if (t) *t = t0 + n_steps;
    return 0;
}

}  // namespace
