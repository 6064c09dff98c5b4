// The aligned ("diagonal") cross block of the decoder (reference: TransformerAlignedDecoderLayerCustom,
// VQCPCB/transformer/transformer_custom.py:389-492).  The layer has no cross-attention: an MLP on the memory gives, per code,
// one row C[b * S + s][j * nc + v] (feature j of voice v), and target token t = event * nc + voice of sequence b receives
// C[b * S + t / U][(.) * nc + t % nc], U = epc * nc target tokens per code.  All kernels here move or add fp32 words:
//   * aligned_expand: one workgroup per (sequence, code) reads the code's C row once (contiguous), turns it voice-major in
//     LDS and writes the code's up to U target rows, which are contiguous in `out`;
//   * aligned_reduce: its transpose for whole sequences; a thread sums the epc events of one (voice, feature) in ascending
//     order (each event's nc * d words are contiguous), LDS turns the sums feature-major and the C-gradient row goes out
//     contiguously;
//   * elu_fwd / elu_bwd: the MLP's activation on (n * S, 2d) -- expm1 / exp evaluated in double and rounded once (the
//     tensor is a sixteenth of the target rows: the fp64 rate cannot be measured here, util.hip's SELU does the same);
//   * decode_aligned_add: the generation step's form, one row per sequence at the position read from device memory.
// No atomics, fixed summation order, no allocation or synchronisation in the launch functions (graph-capture safe).
#include <algorithm>

#include "common.h"

namespace vq {

constexpr int kAlignedThreads = 256;
constexpr int64_t kAlignedMaxRowFloats = 16384;      // nc * d words of one C row in LDS (64 KiB)

// lds[v * d + j] = crow[j * nc + v]
__device__ __forceinline__ void load_c_row_voice_major(const float* __restrict__ crow, float* __restrict__ lds, int nc, int d,
                                                       bool vec) {
    const int w = nc * d;
    if (vec) {
        for (int k = 4 * threadIdx.x; k < w; k += 4 * kAlignedThreads) {
            const float4 c = *reinterpret_cast<const float4*>(crow + k);
            const float e[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) lds[((k + i) % nc) * d + (k + i) / nc] = e[i];
        }
    } else {
        for (int k = threadIdx.x; k < w; k += kAlignedThreads) lds[(k % nc) * d + k / nc] = crow[k];
    }
}

__global__ __launch_bounds__(kAlignedThreads) void aligned_expand_kernel(const float* __restrict__ C, float* __restrict__ out,
                                                                         int S, int P, int U, int nc, int d, int codes,
                                                                         int vec_c, int vec_o) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x / codes, code = blockIdx.x % codes;
    load_c_row_voice_major(C + ((int64_t)b * S + code) * nc * d, lds, nc, d, vec_c != 0);
    __syncthreads();
    const int rows = min(U, P - code * U);                           // a trailing partial code
    float* __restrict__ o = out + ((int64_t)b * P + (int64_t)code * U) * d;
    if (vec_o) {
        const int d4 = d / 4, total = rows * d4;
        for (int m = threadIdx.x; m < total; m += kAlignedThreads) {
            const int r = m / d4, j = (m % d4) * 4;
            reinterpret_cast<float4*>(o)[m] = *reinterpret_cast<const float4*>(lds + (r % nc) * d + j);
        }
    } else {
        const int total = rows * d;
        for (int m = threadIdx.x; m < total; m += kAlignedThreads) o[m] = lds[((m / d) % nc) * d + m % d];
    }
}

__global__ __launch_bounds__(kAlignedThreads) void aligned_reduce_kernel(const float* __restrict__ g, float* __restrict__ dC,
                                                                         int U, int nc, int d, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int w = nc * d, epc = U / nc;
    const float* __restrict__ gb = g + (int64_t)blockIdx.x * U * d;   // the (U, d) block of this (sequence, code)
    float* __restrict__ o = dC + (int64_t)blockIdx.x * w;
    if (vec) {
        for (int m = 4 * threadIdx.x; m < w; m += 4 * kAlignedThreads) {       // m = v * d + j, four features of one voice
            float4 a = *reinterpret_cast<const float4*>(gb + m);
            for (int e = 1; e < epc; ++e) {
                const float4 t = *reinterpret_cast<const float4*>(gb + (int64_t)e * w + m);
                a.x += t.x, a.y += t.y, a.z += t.z, a.w += t.w;
            }
            const int v = m / d, j = m % d;
            lds[j * nc + v] = a.x, lds[(j + 1) * nc + v] = a.y, lds[(j + 2) * nc + v] = a.z, lds[(j + 3) * nc + v] = a.w;
        }
        __syncthreads();
        for (int k = 4 * threadIdx.x; k < w; k += 4 * kAlignedThreads)
            *reinterpret_cast<float4*>(o + k) = *reinterpret_cast<const float4*>(lds + k);
    } else {
        for (int m = threadIdx.x; m < w; m += kAlignedThreads) {
            float a = gb[m];
            for (int e = 1; e < epc; ++e) a += gb[(int64_t)e * w + m];
            lds[(m % d) * nc + m / d] = a;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < w; k += kAlignedThreads) o[k] = lds[k];
    }
}

// ELU, alpha = 1 (torch.nn.ELU): x > 0 ? x : expm1(x)
__device__ __forceinline__ float elu_f(float x) { return x > 0.0f ? x : (float)expm1((double)x); }
__device__ __forceinline__ float elu_grad_f(float x, float g) { return x > 0.0f ? g : (float)((double)g * exp((double)x)); }

__global__ __launch_bounds__(256) void elu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int64_t n4) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < n4; i += step) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<float4*>(y)[i] = make_float4(elu_f(v.x), elu_f(v.y), elu_f(v.z), elu_f(v.w));
    }
    for (int64_t i = 4 * n4 + i0; i < n; i += step) y[i] = elu_f(x[i]);                     // scalar tail
}

__global__ __launch_bounds__(256) void elu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                      float* __restrict__ gx, int64_t n, int64_t n4) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < n4; i += step) {
        const float4 v = reinterpret_cast<const float4*>(x)[i], u = reinterpret_cast<const float4*>(g)[i];
        reinterpret_cast<float4*>(gx)[i] =
            make_float4(elu_grad_f(v.x, u.x), elu_grad_f(v.y, u.y), elu_grad_f(v.z, u.z), elu_grad_f(v.w, u.w));
    }
    for (int64_t i = 4 * n4 + i0; i < n; i += step) gx[i] = elu_grad_f(x[i], g[i]);
}

__global__ __launch_bounds__(256) void decode_aligned_add_kernel(const float* __restrict__ h, int64_t ldh,
                                                                 const float* __restrict__ C, float* __restrict__ s,
                                                                 int64_t lds_, const int32_t* __restrict__ pos, int S, int U,
                                                                 int nc, int d) {
    const int p = pos[0];
    if (p < 0 || p >= S * U) return;                                 // block-uniform; as the step's other kernels past the end
    const int b = blockIdx.x, v = p % nc;
    const float* __restrict__ crow = C + ((int64_t)b * S + p / U) * nc * d;
    for (int j = threadIdx.x; j < d; j += 256) s[b * lds_ + j] = h[b * ldh + j] + crow[(int64_t)j * nc + v];
}

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_aligned_expand(const float* C, float* out, int64_t n, int S, int P, int U, int nc, int d, void* stream) {
    VQ_REQUIRE(n >= 0 && S >= 1 && P >= 0 && U >= 1 && nc >= 1 && d >= 1 && U % nc == 0 && P <= (int64_t)S * U,
               "aligned_expand: need U %% nc == 0 and 0 <= P <= S * U (n=%lld S=%d P=%d U=%d nc=%d d=%d)", (long long)n, S, P, U,
               nc, d);
    VQ_REQUIRE((int64_t)nc * d <= kAlignedMaxRowFloats, "aligned_expand: nc * d <= %lld", (long long)kAlignedMaxRowFloats);
    if (n == 0 || P == 0) return VQCPC_OK;
    VQ_REQUIRE(C && out, "aligned_expand: null pointer");
    const int codes = (int)ceil_div(P, U);
    VQ_REQUIRE(n * codes <= 0x7FFFFFFF, "aligned_expand: too many (sequence, code) pairs");
    const int vec_c = ((int64_t)nc * d) % 4 == 0 && aligned16(C), vec_o = d % 4 == 0 && aligned16(out);
    hipLaunchKernelGGL(aligned_expand_kernel, dim3((unsigned)(n * codes)), dim3(kAlignedThreads), (size_t)nc * d * sizeof(float),
                       (hipStream_t)stream, C, out, S, P, U, nc, d, codes, vec_c, vec_o);
    VQ_CHECK_LAUNCH("aligned_expand");
    return VQCPC_OK;
}

int vqcpc_aligned_reduce(const float* d_out, float* d_C, int64_t n, int S, int U, int nc, int d, void* stream) {
    VQ_REQUIRE(n >= 0 && S >= 1 && U >= 1 && nc >= 1 && d >= 1 && U % nc == 0,
               "aligned_reduce: need U %% nc == 0 (n=%lld S=%d U=%d nc=%d d=%d)", (long long)n, S, U, nc, d);
    VQ_REQUIRE((int64_t)nc * d <= kAlignedMaxRowFloats, "aligned_reduce: nc * d <= %lld", (long long)kAlignedMaxRowFloats);
    if (n == 0) return VQCPC_OK;
    VQ_REQUIRE(d_out && d_C, "aligned_reduce: null pointer");
    VQ_REQUIRE(n * S <= 0x7FFFFFFF, "aligned_reduce: too many (sequence, code) pairs");
    const int vec = d % 4 == 0 && aligned16(d_out) && aligned16(d_C);
    hipLaunchKernelGGL(aligned_reduce_kernel, dim3((unsigned)(n * S)), dim3(kAlignedThreads), (size_t)nc * d * sizeof(float),
                       (hipStream_t)stream, d_out, d_C, U, nc, d, vec);
    VQ_CHECK_LAUNCH("aligned_reduce");
    return VQCPC_OK;
}

int vqcpc_elu_fwd(const float* x, float* y, int64_t n, void* stream) {
    if (n == 0) return VQCPC_OK;
    VQ_REQUIRE(x && y && n >= 0, "elu_fwd: bad arguments");
    const int64_t n4 = aligned16(x) && aligned16(y) ? n / 4 : 0;
    const int blocks = (int)std::min<int64_t>(ceil_div(std::max<int64_t>(n4, n - 4 * n4), 256), 4096);
    hipLaunchKernelGGL(elu_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, n, n4);
    VQ_CHECK_LAUNCH("elu_fwd");
    return VQCPC_OK;
}

int vqcpc_elu_bwd(const float* x, const float* g_out, float* g_x, int64_t n, void* stream) {
    if (n == 0) return VQCPC_OK;
    VQ_REQUIRE(x && g_out && g_x && n >= 0, "elu_bwd: bad arguments");
    const int64_t n4 = aligned16(x) && aligned16(g_out) && aligned16(g_x) ? n / 4 : 0;
    const int blocks = (int)std::min<int64_t>(ceil_div(std::max<int64_t>(n4, n - 4 * n4), 256), 4096);
    hipLaunchKernelGGL(elu_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, g_out, g_x, n, n4);
    VQ_CHECK_LAUNCH("elu_bwd");
    return VQCPC_OK;
}

int vqcpc_decode_aligned_add(const float* h, int64_t ldh, const float* C, float* s, int64_t lds, const int32_t* pos, int64_t M,
                             int S, int U, int nc, int d, void* stream) {
    VQ_REQUIRE(h && C && s && pos && M >= 1 && M <= 64 && S >= 1 && U >= 1 && nc >= 1 && d >= 1 && U % nc == 0 && ldh >= d &&
                   lds >= d,
               "decode_aligned_add: bad arguments (M=%lld S=%d U=%d nc=%d d=%d)", (long long)M, S, U, nc, d);
    hipLaunchKernelGGL(decode_aligned_add_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, h, ldh, C, s, lds, pos, S,
                       U, nc, d);
    VQ_CHECK_LAUNCH("decode_aligned_add");
    return VQCPC_OK;
}

}  // extern "C"
