// Particle resampling for constrained generation (decoders/generation.py; the rule is stated once, in numpy, in
// tests/particles_reference.py).  The M <= 64 rows of an incremental stack are G = M / P groups of P consecutive rows
// ("particles" of one user row).  After every generated code:
//   * vqcpc_particle_resample: ONE workgroup, a wavefront per group, lane j = member j.  Adds the code's forced log-probabilities
//     / allowed masses to the running log-weights, normalises them, and where the effective sample size fell below the
//     threshold draws P ancestors by systematic resampling.  Every sum over the members is sequential in ascending member
//     order and this file is compiled with -ffp-contract=off, so the ancestors are an exact function of the stored weights.
//   * vqcpc_particle_permute_{i64,f32,cache}: row k of a group <- row ancestors[k], IN PLACE.  Ancestor maps contain cycles
//     (a swap) and fan-outs, so a workgroup owns a column tile across ALL rows of a group: it loads the rows that some other
//     row descends from into LDS, and stores only after the barrier behind the last load.  Rows are far apart (a cache row is
//     W * d floats), columns are contiguous: the tile runs along the columns, 16 bytes per lane on the cache path, and is as wide
//     as 32 KiB of LDS allow for the group's P rows.
// The kernels know nothing of the decoder: plain buffers, leading dimensions, the device counters `pos` and `win`.
#include "common.h"

namespace vq {

constexpr int kPartMaxRows = 64;
constexpr int kPartWaves = 16;               // resample: groups per pass of the one workgroup
constexpr int kPermThreads = 256;
constexpr int kPermSlots = 2048;             // permute: elements of the vector type in a workgroup's LDS tile (32 KiB of uint4)
constexpr int kPermLanes = 32;               // lanes along the columns: 512 contiguous bytes per row on the cache path
// the column tile of a group of P rows: the LDS tile holds P x cols, cols a multiple of kPermLanes (P = 64: 32, P = 4: 512) --
// small groups get wide tiles, so that a workgroup always moves up to 32 KiB and the launch is not a swarm of tiny workgroups
static inline __host__ __device__ int perm_cols(int P) { return (kPermSlots / P) / kPermLanes * kPermLanes; }
constexpr uint64_t kPartSeedMul = 0x8CB92BA72F3D8DD7ull;      // the uniform's key, next to vqcpc_decode_window's 0xD1B54A32D192ED03

__device__ __forceinline__ uint64_t part_splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(64 * kPartWaves) void particle_resample_kernel(
    float* __restrict__ lw, float* __restrict__ evidence, float* __restrict__ pending, const int64_t* __restrict__ seeds,
    const int64_t* __restrict__ constraint, int64_t ldcons, const float* __restrict__ logp, int64_t ldlogp,
    const float* __restrict__ logmass, int64_t ldmass, const int32_t* __restrict__ posp, const int32_t* __restrict__ win, int U,
    float threshold, int force, int32_t* __restrict__ ancestors, float* __restrict__ wn_out, float* __restrict__ ess_out,
    int32_t* __restrict__ flag, int32_t* __restrict__ hist_anc, float* __restrict__ hist_wn, float* __restrict__ hist_ess,
    int64_t hist_rows, int M, int P) {
    __shared__ int moved;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = M / P;
    const int w0 = win ? win[1] : 0;
    const int pos = *posp;
    // the chorale index of the code whose U steps have just run
    const int64_t c = (w0 >= 0 && pos >= U) ? (int64_t)w0 + pos / U - 1 : -1;
    if (threadIdx.x == 0) moved = 0;
    __syncthreads();
    const float ninf = -INFINITY;
    for (int g = wave; g < G; g += kPartWaves) {              // a wave's own trip count: no barrier inside
        const int base = g * P;
        const bool mem = lane < P;
        const int b = base + (mem ? lane : 0);
        if (c < 0) {                                          // no finished code (uniform): nothing but the identity map
            if (mem) ancestors[b] = b;
            continue;
        }
        float l = ninf;
        if (mem) {
            l = lw[b];
            for (int j = 0; j < U; ++j) {                     // ascending position order, one fp32 add per addend
                const int64_t q = c * U + j;
                if (constraint && q < ldcons && constraint[(int64_t)b * ldcons + q] >= 0) {
                    if (logp && q < ldlogp) l = l + logp[(int64_t)b * ldlogp + q];
                } else if (logmass && q < ldmass) {
                    l = l + logmass[(int64_t)b * ldmass + q];
                }
            }
            if (l != l) l = ninf;                             // NaN counts as -inf
        }
        const float mx = wave_max(l);                         // lanes >= P hold -inf
        const bool dead = !(mx > ninf);                       // every member is -inf
        const float w = (mem && !dead && l > ninf) ? expf(l - mx) : 0.0f;
        float s = 0.0f;
        for (int j = 0; j < P; ++j) s = s + __shfl(w, j, 64);
        const float wn = dead ? 1.0f / (float)P : w / s;
        float ss = 0.0f;
        for (int j = 0; j < P; ++j) {
            const float o = __shfl(wn, j, 64);
            ss = ss + o * o;
        }
        const float ess = 1.0f / ss;
        const float inc = dead ? ninf : (mx + logf(s)) - logf((float)P);
        const bool resample = !dead && (force != 0 || ess < threshold * (float)P);
        int a = lane;
        if (resample) {
            const uint64_t key = (uint64_t)seeds[base] ^ ((uint64_t)(c + 1) * kPartSeedMul);
            const float u = (float)(uint32_t)(part_splitmix64(key) >> 40) * (1.0f / 16777216.0f);
            const float target = (u + (float)lane) / (float)P;
            float cum = 0.0f;
            a = P - 1;                                        // none exceeds (the sum rounded below the target): the last member
            bool found = false;
            for (int j = 0; j < P; ++j) {
                cum = cum + __shfl(wn, j, 64);
                if (!found && cum > target) {
                    a = j;
                    found = true;
                }
            }
        }
        if (mem) {
            ancestors[b] = base + a;
            wn_out[b] = wn;
            lw[b] = resample ? 0.0f : l;
            if (c < hist_rows) {
                if (hist_anc) hist_anc[c * M + b] = base + a;
                if (hist_wn) hist_wn[c * M + b] = wn;
            }
            if (a != lane) moved = 1;                         // benign race: every writer stores 1
        }
        if (lane == 0) {
            ess_out[g] = ess;
            pending[g] = inc;
            if (dead) evidence[g] = ninf;
            else if (resample) evidence[g] = evidence[g] + inc;
            if (c < hist_rows && hist_ess) hist_ess[c * G + g] = ess;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *flag = moved;
}

// V: the element the tile moves (uint32_t / uint64_t rows, uint4 = four floats on the aligned paths).  buf: `planes` planes
// of M rows of ld elements; columns [0, cols) move, cols = width, or clamp(pos, 0, width / per_pos) * per_pos with posp.
template <typename V>
__global__ __launch_bounds__(kPermThreads) void particle_permute_kernel(V* __restrict__ buf, int64_t ld, int64_t plane_stride,
                                                                        int64_t width, int64_t per_pos,
                                                                        const int32_t* __restrict__ posp,
                                                                        const int32_t* __restrict__ ancestors,
                                                                        const int32_t* __restrict__ flag, int P) {
    __shared__ V tile[kPermSlots];
    __shared__ int sanc[kPartMaxRows];
    __shared__ int sneed[kPartMaxRows];
    if (*flag == 0) return;                                   // nothing moved anywhere (uniform)
    int64_t cols = width;
    if (posp) cols = min(max((int64_t)*posp, (int64_t)0), width / per_pos) * per_pos;
    const int tc = perm_cols(P);
    const int64_t c0 = (int64_t)blockIdx.x * tc;
    if (c0 >= cols) return;                                   // uniform
    const int n = (int)min((int64_t)tc, cols - c0);
    const int tid = threadIdx.x;
    const int base = blockIdx.y * P;
    if (tid < kPartMaxRows) sneed[tid] = 0;
    __syncthreads();
    if (tid < P) {
        int a = ancestors[base + tid] - base;
        if (a < 0 || a >= P) a = tid;                         // a map that leaves the group is no map: the row stays
        sanc[tid] = a;
        if (a != tid) sneed[a] = 1;                           // benign race: every writer stores 1
    }
    __syncthreads();
    V* __restrict__ b = buf + (int64_t)blockIdx.z * plane_stride + (int64_t)base * ld + c0;
    const int cx = tid % kPermLanes, ry = tid / kPermLanes;   // 8 rows per pass, 32 lanes along the columns
    for (int r = ry; r < P; r += kPermThreads / kPermLanes) {
        if (!sneed[r]) continue;                              // nobody else descends from this row
        for (int c = cx; c < n; c += kPermLanes) tile[r * tc + c] = b[(int64_t)r * ld + c];
    }
    __syncthreads();                                          // every load of the tile is done: the stores may overwrite
    for (int r = ry; r < P; r += kPermThreads / kPermLanes) {
        const int a = sanc[r];
        if (a == r) continue;
        for (int c = cx; c < n; c += kPermLanes) b[(int64_t)r * ld + c] = tile[a * tc + c];
    }
}

template <typename V>
static int permute_launch(const char* name, V* buf, int64_t ld, int64_t planes, int64_t plane_stride, int64_t width,
                          int64_t per_pos, const int32_t* pos, const int32_t* ancestors, const int32_t* flag, int64_t M, int P,
                          void* stream) {
    if (width == 0) return VQCPC_OK;
    const dim3 grid((unsigned)ceil_div(width, perm_cols(P)), (unsigned)(M / P), (unsigned)planes), block(kPermThreads);
    hipLaunchKernelGGL((particle_permute_kernel<V>), grid, block, 0, (hipStream_t)stream, buf, ld, plane_stride, width, per_pos,
                       pos, ancestors, flag, P);
    VQ_CHECK_LAUNCH(name);
    return VQCPC_OK;
}

static bool groups_ok(int64_t M, int P) { return M >= 1 && M <= kPartMaxRows && P >= 2 && P <= kPartMaxRows && M % P == 0; }

}  // namespace vq

using namespace vq;

extern "C" {

int vqcpc_particle_resample(float* lw, float* evidence, float* pending, const int64_t* seeds, const int64_t* constraint,
                            int64_t ldcons, const float* logp, int64_t ldlogp, const float* logmass, int64_t ldmass,
                            const int32_t* pos, const int32_t* win, int U, float threshold, int force, int32_t* ancestors,
                            float* wn, float* ess, int32_t* flag, int32_t* hist_ancestors, float* hist_wn, float* hist_ess,
                            int64_t hist_rows, int64_t M, int P, void* stream) {
    VQ_REQUIRE(lw && evidence && pending && seeds && pos && ancestors && wn && ess && flag && groups_ok(M, P),
               "particle_resample: bad arguments (1 <= M <= 64, 2 <= P <= 64, M %% P == 0)");
    VQ_REQUIRE(U >= 1 && threshold >= 0.0f && threshold <= 1.0f && hist_rows >= 0 && (!constraint || ldcons >= 1) &&
               (!logp || ldlogp >= 1) && (!logmass || ldmass >= 1),
               "particle_resample: U >= 1, 0 <= threshold <= 1, leading dimensions >= 1");
    hipLaunchKernelGGL(particle_resample_kernel, dim3(1), dim3(64 * kPartWaves), 0, (hipStream_t)stream, lw, evidence, pending,
                       seeds, constraint, ldcons, logp, ldlogp, logmass, ldmass, pos, win, U, threshold, force, ancestors, wn, ess,
                       flag, hist_ancestors, hist_wn, hist_ess, hist_rows, (int)M, P);
    VQ_CHECK_LAUNCH("particle_resample");
    return VQCPC_OK;
}

int vqcpc_particle_permute_i64(int64_t* buf, int64_t ld, int64_t width, const int32_t* pos, const int32_t* ancestors,
                               const int32_t* flag, int64_t M, int P, void* stream) {
    VQ_REQUIRE(buf && ancestors && flag && groups_ok(M, P) && width >= 0 && ld >= width,
               "particle_permute_i64: bad arguments (1 <= M <= 64, 2 <= P <= 64, M %% P == 0, ld >= width >= 0)");
    return permute_launch("particle_permute_i64", reinterpret_cast<uint64_t*>(buf), ld, 1, 0, width, 1, pos, ancestors, flag, M, P,
                          stream);
}

int vqcpc_particle_permute_f32(float* buf, int64_t ld, int64_t width, const int32_t* pos, const int32_t* ancestors,
                               const int32_t* flag, int64_t M, int P, void* stream) {
    VQ_REQUIRE(buf && ancestors && flag && groups_ok(M, P) && width >= 0 && ld >= width,
               "particle_permute_f32: bad arguments (1 <= M <= 64, 2 <= P <= 64, M %% P == 0, ld >= width >= 0)");
    if (!pos && width % 4 == 0 && ld % 4 == 0 && aligned16(buf))
        return permute_launch("particle_permute_f32", reinterpret_cast<uint4*>(buf), ld / 4, 1, 0, width / 4, 1, pos, ancestors,
                              flag, M, P, stream);
    return permute_launch("particle_permute_f32", reinterpret_cast<uint32_t*>(buf), ld, 1, 0, width, 1, pos, ancestors, flag, M, P,
                          stream);
}

int vqcpc_particle_permute_cache(float* cache, int layers, int64_t W, int d, const int32_t* pos, const int32_t* ancestors,
                                 const int32_t* flag, int64_t M, int P, void* stream) {
    VQ_REQUIRE(cache && pos && ancestors && flag && groups_ok(M, P) && layers >= 1 && layers <= 65535 && W >= 1 && d >= 4 &&
               d % 4 == 0 && aligned16(cache),
               "particle_permute_cache: bad arguments (1 <= M <= 64, 2 <= P <= 64, M %% P == 0, d %% 4 == 0, 16-byte aligned)");
    const int64_t ld = W * (d / 4);
    return permute_launch("particle_permute_cache", reinterpret_cast<uint4*>(cache), ld, layers, M * ld, ld, d / 4, pos, ancestors,
                          flag, M, P, stream);
}

}  // extern "C"
