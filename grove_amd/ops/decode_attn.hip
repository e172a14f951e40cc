// decode_attn — split-KV GQA decode attention for MI355X (gfx950/CDNA4).
//
//   out[b,h,:] = softmax_j(scale * q[b,h,:] . k[b,h/G,j,:]) . v[b,h/G,j,:],  j < seq_lens[b]
//
// One query token per sequence, head dim 128, bf16 in / fp32 out. The kernel is a
// plain stream over the KV cache: every (sequence, KV head) owns one contiguous
// [Lmax,128] run of K and one of V, read once per step.
//
// Pass 1 (decode_attn_kernel): one single-wave workgroup per (b, kv head, split).
// A split walks its keys in tiles of 32:
//   * S^T = K . Q^T on v_mfma_f32_16x16x32_bf16 with K as the A operand (rows =
//     keys) and the G query heads of the KV head, zero-padded to 16, as the B
//     operand (cols = heads). With the operand lane map (row = lane&15,
//     k = 8*(lane>>4)+j) both are plain 16-B loads from row-major memory; Q is
//     loaded once and stays in registers. Putting the keys on the ROW side leaves
//     one head per lane column, so the online softmax (running max m and sum l,
//     exp2 with scale*log2(e) folded in) needs two xor-shuffles per tile and the
//     bf16 P fragment of the second product is lane-local: no transpose of P.
//     MFMA row r of 16-key group t is key 8*(r>>2) + 4*t + (r&3) of the tile, which
//     makes lane group g own keys 8g..8g+7 in natural order.
//   * O^T += V^T . P^T, again 16x16x32 (rows = 16 of the 128 dims, contraction
//     over the 32 keys). This is the operand that needs transposing: V goes
//     global -> VGPR -> LDS (row-major 256-B rows, 16-B chunks XOR-swizzled) and is
//     read back with ds_read_b64_tr_b16, which hands each lane four keys of one
//     dim. The two 4-key blocks a 32-lane half reads sit 8 rows apart and the
//     swizzle spreads their 16 chunks over all 64 banks. The instruction needs
//     EXEC all ones: the key loop's trip count is wave-uniform and nothing inside
//     it branches on the lane.
//   * K and V both go through a buffer descriptor that ends at the split's last
//     valid key, min(seq_len, split end): rows past it are never fetched and come
//     back as zeros with no branch around the loads, so the tile after the last
//     can be prefetched unconditionally. Scores of keys past the end are set to
//     -inf before the max. K is prefetched one tile ahead into a second register
//     set (two tiles per loop trip, statically named sets, so the waits are
//     counted vmcnt); V of tile n+1 is requested as soon as tile n is in LDS.
//   * splits == 1 normalises and writes out; otherwise the split writes its
//     unnormalised (m, l, O[16x128]) to an fp32 workspace.
// Pass 2 (decode_attn_combine_kernel) merges the splits of one (b, h) in split
// order, skipping empty ones (l == 0, m == -inf), and normalises. No atomics:
// two calls give bit-identical results. A length of 0 gives zeros.
//
// P.V on the VALU (lanes owning d-slices) was not built: at G = 1 the MFMA path
// does 16x the useful FLOPs and still idles behind the KV stream (see
// docs/benchmarks.md), so there was nothing for a second path to win.
#include <torch/extension.h>
#include <ATen/DeviceGuard.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>
#include <chrono>
#include <cmath>

namespace {

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

constexpr int DA_D = 128;          // head dim
constexpr int DA_TILE = 32;        // keys per tile (one PV contraction)
constexpr int DA_ROW = DA_D * 2;   // bytes per key row
constexpr int DA_MAX_SPLITS = 1024;
constexpr int64_t DA_MAX_L = 1 << 22;   // one stream = Lmax*256 B <= 1 GiB: int offsets

// Two waves per SIMD (<= 256 registers): left to itself the compiler hoists every LDS
// address out of the loop, takes 260 and halves the waves a CU can hold.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
void decode_attn_kernel(const bf16* __restrict__ Q,      // [B][Hq][128]
                        const bf16* __restrict__ Kc,     // [B][Hkv][Lmax][128]
                        const bf16* __restrict__ Vc,     // [B][Hkv][Lmax][128]
                        const int* __restrict__ seq_lens,
                        float* __restrict__ out,         // [B][Hq][128]
                        float* __restrict__ ws_o,        // [B*Hkv][splits][16][128]
                        float* __restrict__ ws_ml,       // [B*Hkv][splits][16][2]
                        int Hkv, int G, int Lmax, int splits, int chunk,
                        float scale_log2e) {
    __shared__ __attribute__((aligned(16))) unsigned char vs[DA_TILE * DA_ROW];
    const int lane = threadIdx.x;
    const int r = lane & 15, g = lane >> 4;
    const int sp = blockIdx.x % splits;
    const int bh = blockIdx.x / splits;                  // b*Hkv + kv head
    const int b = bh / Hkv, kvh = bh - b * Hkv;
    const int len = min(max(seq_lens[b], 0), Lmax);
    const int lo = sp * chunk;
    // readfirstlane: the compiler picks a vector min3 here, and a descriptor built
    // from a VGPR makes every buffer load a waterfall loop
    const int hi = __builtin_amdgcn_readfirstlane(min(lo + chunk, len));
    const int ntiles = hi > lo ? (hi - lo + DA_TILE - 1) / DA_TILE : 0;

    // descriptors end at key hi: an empty split fetches nothing at all
    const long stream = (long)bh * Lmax * DA_D;
    const int nrec = hi > lo ? hi * DA_ROW : 0;
    const auto krs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16*>(Kc + stream), /*stride*/0, nrec, 0x00020000);
    const auto vrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16*>(Vc + stream), /*stride*/0, nrec, 0x00020000);

    // Q fragments: head r of this KV head's group, zero for the padding heads
    bf16x8 qf[4] = {};
    if (r < G) {
        const bf16x8* qp = (const bf16x8*)(
            Q + ((long)(b * Hkv + kvh) * G + r) * DA_D + 8 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            qf[i] = qp[4 * i];
    }

    // K: MFMA row r of key group t is key 8*(r>>2) + 4t + (r&3) of the tile
    const unsigned klane = (unsigned)((8 * (r >> 2) + (r & 3)) * DA_ROW + 16 * g);
    // V: load i covers keys 4i..4i+3 of the tile, lane group g one 256-B row each
    const unsigned vlane = (unsigned)(g * DA_ROW + 16 * r);
    // LDS image: off(row, ch) = 256*row + 16*(ch ^ (((row&3)<<2) | ((row>>2)&3)))
    const unsigned wlane = (unsigned)(g * DA_ROW);       // row = 4i + g, chunk r
    const unsigned wxor = (unsigned)(g << 2);            // | (i & 3) per load
    // transposed read of dims 16dt..16dt+15, keys 8g+4t..8g+4t+3: lane 4q+p of the
    // group supplies off(8g+4t+q, 2dt + (p>>1)) + 8*(p&1)
    const int tq = r >> 2, tp = r & 3;

    auto load_k = [&](bf16x8 (&k)[2][4], int tile) {
        // the whole offset rides in voffset, the part the range check surely covers
        const unsigned off = klane + (unsigned)((lo + tile * DA_TILE) * DA_ROW);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                k[t][i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                    krs, off + t * (4 * DA_ROW) + i * 64, 0, 0));
    };
    bf16x8 vr[8];
    auto load_v = [&](int tile) {
        const unsigned off = vlane + (unsigned)((lo + tile * DA_TILE) * DA_ROW);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            vr[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                vrs, off + i * (4 * DA_ROW), 0, 0));
    };

    float m = -INFINITY, l = 0.f;      // m is the same in the four lanes of a head;
    f32x4 acc[8] = {};                 // l is this lane's share until the epilogue

    auto step = [&](const bf16x8 (&k)[2][4], int tile) {
        f32x4 s[2] = {};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t)
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k[t][i], qf[i], s[t], 0, 0, 0);
        // C/D map: col = lane&15 -> head, row = 4g + e -> key 8g + 4t + e
        const int key0 = lo + tile * DA_TILE + 8 * g;
        float p[8];
        float tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = s[j >> 2][j & 3] * scale_log2e;
            p[j] = key0 + j < hi ? v : -INFINITY;
            tmax = fmaxf(tmax, p[j]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        // every tile holds at least one key below hi, so m_new is finite and
        // neither exp2 below sees (-inf) - (-inf)
        const float m_new = fmaxf(m, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);
        m = m_new;
        float psum = 0.f;
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            p[j] = __builtin_amdgcn_exp2f(p[j] - m_new);
            psum += p[j];                  // l sums the unrounded p
            pf[j] = (__bf16)p[j];
        }
        l = l * alpha + psum;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
            acc[dt] *= alpha;

        // V of this tile -> LDS, then its registers take the next tile's loads
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *(bf16x8*)(vs + i * (4 * DA_ROW) + wlane
                       + 16 * ((unsigned)r ^ wxor ^ (unsigned)(i & 3))) = vr[i];
        load_v(tile + 1);
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            bf16x4 h[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int row = 8 * g + 4 * t + tq;
                const int ch = (2 * dt + (tp >> 1)) ^ ((tq << 2) | ((2 * g + t) & 3));
                h[t] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_bf16x4*)(vs + row * DA_ROW + 16 * ch + 8 * (tp & 1)));
            }
            bf16x8 vf = __builtin_shufflevector(h[0], h[1], 0, 1, 2, 3, 4, 5, 6, 7);
            // A = V^T (row = dim 16dt + lane&15, k = key 8g+j), B = P^T (col = head)
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[dt], 0, 0, 0);
        }
    };

    bf16x8 k0[2][4], k1[2][4];
    load_k(k0, 0);
    load_v(0);
    int t = 0;
    for (; t + 2 <= ntiles; t += 2) {
        load_k(k1, t + 1);
        step(k0, t);
        load_k(k0, t + 2);
        step(k1, t + 1);
    }
    if (t < ntiles)                    // wave-uniform: EXEC stays all ones inside
        step(k0, t);

    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    // C/D map: col = lane&15 -> head, row = 4g + e -> dim 16dt + 4g + e
    if (r < G) {
        if (splits == 1) {
            const float inv = l > 0.f ? 1.f / l : 0.f;
            float* o = out + ((long)(b * Hkv + kvh) * G + r) * DA_D + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
                *(f32x4*)(o + 16 * dt) = acc[dt] * inv;
        } else {
            const long slot = ((long)bh * splits + sp) * 16 + r;
            float* o = ws_o + slot * DA_D + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
                *(f32x4*)(o + 16 * dt) = acc[dt];
            if (g == 0) {
                ws_ml[slot * 2] = m;
                ws_ml[slot * 2 + 1] = l;
            }
        }
    }
}

// One workgroup per (b, query head), one thread per dim. The threads first share out
// the (m, l) pairs: M is the max over the non-empty splits (a max does not depend on
// its order) and split s gets the weight w_s = exp2(m_s - M), or 0 when it is empty
// (l == 0, m == -inf), so exp2 only ever sees finite m_s and M. Then every thread
// sums w_s * l_s and w_s * O_s[d] over s in split order. The O loads do not depend
// on one another, so the loop keeps eight in flight. (Measured: the first version
// walked the splits with a branch per split and dependent loads, ~0.5 us per split;
// at B=1, 8192 tokens, 256 splits it took 160 us of a 165 us step.)
__global__ __launch_bounds__(DA_D)
void decode_attn_combine_kernel(const float* __restrict__ ws_o,
                                const float* __restrict__ ws_ml,
                                float* __restrict__ out, int Hkv, int G, int splits) {
    __shared__ float w_sh[DA_MAX_SPLITS], wl_sh[DA_MAX_SPLITS], red[2];
    const int hq = blockIdx.x % (Hkv * G);
    const int b = blockIdx.x / (Hkv * G);
    const int kvh = hq / G, r = hq - kvh * G;
    const long slot0 = ((long)(b * Hkv + kvh) * splits) * 16 + r;
    const int d = threadIdx.x;
    float lm = -INFINITY;
    for (int s = d; s < splits; s += DA_D) {
        const float* ml = ws_ml + (slot0 + (long)s * 16) * 2;
        if (ml[1] > 0.f) lm = fmaxf(lm, ml[0]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        lm = fmaxf(lm, __shfl_xor(lm, off));
    if ((d & 63) == 0) red[d >> 6] = lm;
    __syncthreads();
    const float M = fmaxf(red[0], red[1]);
    for (int s = d; s < splits; s += DA_D) {
        const float* ml = ws_ml + (slot0 + (long)s * 16) * 2;
        const float ls = ml[1];
        const float w = ls > 0.f ? __builtin_amdgcn_exp2f(ml[0] - M) : 0.f;
        w_sh[s] = w;
        wl_sh[s] = w * ls;
    }
    __syncthreads();
    const float* op = ws_o + slot0 * DA_D + d;
    float o = 0.f, L = 0.f;
#pragma unroll 8
    for (int s = 0; s < splits; ++s) {
        o += w_sh[s] * op[(long)s * 16 * DA_D];   // an empty split wrote O = 0
        L += wl_sh[s];
    }
    out[(long)blockIdx.x * DA_D + d] = L > 0.f ? o / L : 0.f;
}

void check_decode_attn_dims(int64_t B, int64_t Hq, int64_t Hkv, int64_t Lmax,
                            int64_t D, int64_t splits) {
    TORCH_CHECK(D == DA_D, "decode_attn_bf16 requires head dim 128 (got ", D, ")");
    TORCH_CHECK(B >= 1 && Hq >= 1 && Hkv >= 1 && Lmax >= 1 && Lmax <= DA_MAX_L,
                "decode_attn_bf16 requires B>=1, heads>=1, 1<=Lmax<=", DA_MAX_L,
                " (got B=", B, " Hq=", Hq, " Hkv=", Hkv, " Lmax=", Lmax, ")");
    TORCH_CHECK(Hq % Hkv == 0, "Hq must be a multiple of Hkv (got Hq=", Hq,
                " Hkv=", Hkv, ")");
    const int64_t G = Hq / Hkv;
    TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8 || G == 16,
                "Hq/Hkv must be 1, 2, 4, 8 or 16 (got ", G, ")");
    TORCH_CHECK(splits >= 0 && splits <= DA_MAX_SPLITS,
                "splits must be 0 (auto) or 1..", DA_MAX_SPLITS, " (got ", splits, ")");
    TORCH_CHECK(B * Hq <= INT32_MAX / DA_MAX_SPLITS,
                "B*Hq too large for the grid (got B=", B, " Hq=", Hq, ")");
}

// Keys per split for a given split count: a multiple of the key tile.
int64_t decode_attn_chunk(int64_t Lmax, int64_t splits) {
    int64_t chunk = (Lmax + splits - 1) / splits;
    return (chunk + DA_TILE - 1) / DA_TILE * DA_TILE;
}

void launch_decode_attn(const bf16* q, const bf16* k, const bf16* v, const int* lens,
                        float* out, float* ws_o, float* ws_ml, int64_t B, int64_t Hq,
                        int64_t Hkv, int64_t Lmax, int64_t splits, float scale,
                        hipStream_t stream) {
    const int G = (int)(Hq / Hkv);
    const int chunk = (int)decode_attn_chunk(Lmax, splits);
    const float scale_log2e = scale * 1.4426950408889634f;
    hipLaunchKernelGGL(decode_attn_kernel, dim3((unsigned)(B * Hkv * splits)), dim3(64),
                       0, stream, q, k, v, lens, out, ws_o, ws_ml, (int)Hkv, G,
                       (int)Lmax, (int)splits, chunk, scale_log2e);
    if (splits > 1)
        hipLaunchKernelGGL(decode_attn_combine_kernel, dim3((unsigned)(B * Hq)),
                           dim3(DA_D), 0, stream, ws_o, ws_ml, out, (int)Hkv, G,
                           (int)splits);
}

}  // namespace

// Splits per (sequence, KV head), from the shape alone (never from the lengths, so
// the choice is reproducible and needs no sync). A split is one wave. One wave alone
// streams ~16 GB/s (it has one 16-KB tile in flight), so the grid has to be wide, but
// every split costs an 8-KB workspace round trip and a share of the combine pass, so
// not wider than needed. Measured on one MI355X, Hq=64 Hkv=8, KV GB/s by split count
// (waves = B*Hkv*splits):
//   ctx 8192  B=1  :   8: 1130   16: 1776   32: 2442   64: 2582  128: 1997  256: 1324
//   ctx 8192  B=4  :   8: 4190   16: 5431   32: 5129   64: 4751  128: 4066
//   ctx 8192  B=8  :   8: 5820   16: 6060   32: 5774   64: 5501
//   ctx 8192  B=32 :   2: 5485    4: 5698    8: 5541   16: 5358   32: 4975   64: 4718
//   ctx 8192  B=128:   1: 6263    2: 6328    4: 6277    8: 6158
//   ctx 32768 B=1  :  32: 4051   64: 4937  128: 4345  256: 3532  512: 2535
//   ctx 1024  B=32 :   1: 4629    2: 5199    4: 5053    8: 4957
//   Hq=8 Hkv=1 ctx 2048 B=8:  1: 216   4: 552   8: 827   16: 997   32: 1028
// The best column has 512 to 1024 waves in every row, and splits shorter than 128
// keys lose wherever they were tried except the last row (+3%). 512 waves is within
// 4% of the best of every row; 1024 loses 12% at ctx 32768 B=1 and 6% at B=4.
constexpr int64_t DA_TARGET_WAVES = 512;
constexpr int64_t DA_MIN_KEYS = 128;

int64_t decode_attn_splits(int64_t batch, int64_t hkv, int64_t lmax) {
    TORCH_CHECK(batch >= 1 && hkv >= 1 && lmax >= 1, "batch, hkv, lmax must be >= 1");
    int64_t want = (DA_TARGET_WAVES + batch * hkv - 1) / (batch * hkv);
    int64_t cap = std::max<int64_t>(1, lmax / DA_MIN_KEYS);
    int64_t splits = std::min<int64_t>(std::min(want, cap), DA_MAX_SPLITS);
    // drop splits that the tile rounding of the chunk would leave empty
    int64_t chunk = decode_attn_chunk(lmax, splits);
    return (lmax + chunk - 1) / chunk;
}

torch::Tensor decode_attn_bf16(torch::Tensor q, torch::Tensor k_cache,
                               torch::Tensor v_cache, torch::Tensor seq_lens,
                               double scale, int64_t splits) {
    TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda()
                && seq_lens.is_cuda(), "q, k_cache, v_cache, seq_lens must be on GPU");
    TORCH_CHECK(q.get_device() == k_cache.get_device()
                && q.get_device() == v_cache.get_device()
                && q.get_device() == seq_lens.get_device(),
                "q, k_cache, v_cache, seq_lens must be on one device");
    TORCH_CHECK(q.dtype() == torch::kBFloat16 && k_cache.dtype() == torch::kBFloat16
                && v_cache.dtype() == torch::kBFloat16, "q, k_cache, v_cache must be bf16");
    TORCH_CHECK(seq_lens.dtype() == torch::kInt32, "seq_lens must be int32");
    TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4 && v_cache.dim() == 4
                && seq_lens.dim() == 1,
                "q must be [B,Hq,128], caches [B,Hkv,Lmax,128], seq_lens [B]");
    TORCH_CHECK(q.is_contiguous() && k_cache.is_contiguous() && v_cache.is_contiguous()
                && seq_lens.is_contiguous(), "contiguous required");
    const int64_t B = q.size(0), Hq = q.size(1), Hkv = k_cache.size(1),
                  Lmax = k_cache.size(2);
    TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), "k_cache and v_cache shapes differ");
    TORCH_CHECK(k_cache.size(0) == B && seq_lens.size(0) == B,
                "batch mismatch between q, the caches and seq_lens");
    TORCH_CHECK(q.size(2) == k_cache.size(3), "head dim mismatch between q and the caches");
    check_decode_attn_dims(B, Hq, Hkv, Lmax, q.size(2), splits);
    TORCH_CHECK(std::isfinite(scale) && scale >= 0.0, "scale must be finite and >= 0");
    if (scale == 0.0) scale = 1.0 / std::sqrt((double)DA_D);
    if (!splits) splits = decode_attn_splits(B, Hkv, Lmax);

    const at::DeviceGuard guard(q.device());
    auto fopt = q.options().dtype(torch::kFloat32);
    auto out = torch::empty({B, Hq, DA_D}, fopt);
    torch::Tensor ws_o, ws_ml;
    if (splits > 1) {
        ws_o = torch::empty({B * Hkv, splits, 16, DA_D}, fopt);
        ws_ml = torch::empty({B * Hkv, splits, 16, 2}, fopt);
    }
    launch_decode_attn((const bf16*)q.data_ptr(), (const bf16*)k_cache.data_ptr(),
                       (const bf16*)v_cache.data_ptr(), seq_lens.data_ptr<int>(),
                       out.data_ptr<float>(),
                       splits > 1 ? ws_o.data_ptr<float>() : nullptr,
                       splits > 1 ? ws_ml.data_ptr<float>() : nullptr,
                       B, Hq, Hkv, Lmax, splits, (float)scale,
                       at::hip::getCurrentHIPStream());
    return out;
}

// Long-context decode payload: `iters` attention steps of `batch` sequences, every
// one `ctx` tokens long; returns KV-stream GB/s (K and V are each read once per step).
double burn_decode_attn(int64_t hq, int64_t hkv, int64_t ctx, int64_t batch,
                        int64_t iters, int64_t splits) {
    TORCH_CHECK(hkv >= 1, "hkv must be >= 1");
    check_decode_attn_dims(batch, hq, hkv, ctx, DA_D, splits);
    if (!splits) splits = decode_attn_splits(batch, hkv, ctx);
    auto opt = torch::TensorOptions().dtype(torch::kBFloat16).device(torch::kCUDA);
    auto fopt = opt.dtype(torch::kFloat32);
    auto q = torch::randn({batch, hq, DA_D}, fopt).to(torch::kBFloat16);
    auto k = torch::randn({batch, hkv, ctx, DA_D}, fopt).to(torch::kBFloat16);
    auto v = torch::randn({batch, hkv, ctx, DA_D}, fopt).to(torch::kBFloat16);
    auto lens = torch::full({batch}, ctx, opt.dtype(torch::kInt32));
    auto out = torch::empty({batch, hq, DA_D}, fopt);
    auto ws_o = torch::empty({batch * hkv, splits, 16, DA_D}, fopt);
    auto ws_ml = torch::empty({batch * hkv, splits, 16, 2}, fopt);
    const float scale = 1.f / std::sqrt((float)DA_D);
    hipStream_t stream = at::hip::getCurrentHIPStream();
    auto launch = [&] {
        launch_decode_attn((const bf16*)q.data_ptr(), (const bf16*)k.data_ptr(),
                           (const bf16*)v.data_ptr(), lens.data_ptr<int>(),
                           out.data_ptr<float>(), ws_o.data_ptr<float>(),
                           ws_ml.data_ptr<float>(), batch, hq, hkv, ctx, splits, scale,
                           stream);
    };
    launch();
    C10_HIP_CHECK(hipStreamSynchronize(stream));
    auto t0 = std::chrono::steady_clock::now();
    for (int64_t i = 0; i < iters; ++i) launch();
    C10_HIP_CHECK(hipStreamSynchronize(stream));
    auto t1 = std::chrono::steady_clock::now();
    double secs = std::chrono::duration<double>(t1 - t0).count();
    return 2.0 * batch * hkv * ctx * DA_D * 2.0 * iters / secs / 1e9;  // K+V bytes
}
