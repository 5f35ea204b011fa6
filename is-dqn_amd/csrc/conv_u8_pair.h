// First convolution (uint8 frames, architectures/dqn.py:51-58): ONE workgroup of eight waves per image, the layer's weights resident
// in LDS for the whole image, the image staged in "halves" of two 128-pixel tiles each.
//
// Why (profiles/round3/stamps_u8_pair.txt, profiles/round4/stamps_all.txt, NOTEBOOK 2026-10-20): the previous form -- four waves on a
// pair of tiles, two workgroups per image -- walked the 32 KB of weights through a four-deep global -> register -> LDS ring once per
// TILE (four times per image, one barrier per K step, 64 barriers per image), staged 36 input rows per tile (144 rows for the 84-row
// image, each converted u8 -> bf16 again) and ran all four waves over the last tile's 16 pixels.  Here
//   * the weights (32 rows x 256 k, hi + lo planes) are read from the S8 mirror once per workgroup, two 32-byte chunks per thread, and
//     stay in LDS: the K rotation of a tile is only the LDS column its waves start from, and the K loop has no barrier;
//   * waves 0-3 compute old tile 2h, waves 4-7 old tile 2h + 1 of half h on ONE LDS image of the rows both need (84 x 84: 56 rows for
//     half 0, 40 for half 1: 96 rows per image);
//   * the weights (they need no frame id: they travel under that round trip), the frame rows of half 0 and the frame rows of half 1
//     are requested back to back at the start; half 1's rows wait in registers under half 0's K loop and epilogue (nothing in the
//     K loop loads from global memory any more, so no wait is ordered behind them) and are converted into the (then dead) LDS image
//     behind one barrier;
//   * a wave whose 32 pixel slots all lie past the image skips K loop and epilogue (84 x 84, 21 x 21 pixels: waves 6-7 of half 1), and a
//     wave none of whose 64 positions of a batch lies in the image of the half skips their conversion.
// Three barriers per image.  512 threads at four waves per SIMD (128 registers, no scratch), 75 KB of LDS at 84 x 84: two workgroups
// per CU, the 512 images of the headline step in one round.
// Measured at the headline size (profiles/conv0_image/): 26.3 -> 21.2 us in the traced step, the untraced step +2 %.
//
// The arithmetic is conv_fwd_img_kernel's, statement for statement (same pixel -> lane assignment inside the old tile, same K-step
// rotation per (image, old tile), same pass order, same epilogue): the outputs are bit-identical
// (tests/test_gpu_network.py::test_first_layer_pair_kernel_is_bit_identical_to_the_one_tile_kernel, tests/test_gpu_conv0_image_kernel.py).
// uint8 layers of four stacked frames (K = 256: eight K steps), at most 32 output channels (MT = 2) and an even tile count only.
#pragma once
#include "conv_img.h"

namespace isdqn {

constexpr int U8P_PB = 2;         // positions per thread: one batch covers the image of a half (Rd * Wp / 8 <= 2 * 512 positions)
constexpr int U8P_THREADS = 512;  // eight waves: two groups of four, one old tile each
// Row pitch of the resident weights [32 rows][256 k]: 272 elements = 544 bytes, (pitch / 16) = 2 (mod 4) -- the rule at
// ConvImgTraits::GA -- so the 16-lane groups of a fragment's ds_read_b128 hit 16 distinct bank quads (scripts/lds_conflicts.py:
// 1.0; a pad of 8 elements, (pitch / 16) = 1 (mod 4), gives 2.0 on the third lane group).
constexpr int U8P_WPITCH = 256 + 16;
constexpr int U8P_WPLANE = 32 * U8P_WPITCH;

// K rotation of conv_fwd_img_kernel's workgroup for (image j, old tile): blockIdx / 8 there is (j / 8) * tiles + tile for the images
// of the full groups of eight (xcd_image_tile), the plain workgroup index / 8 in the tail group.
__host__ __device__ __forceinline__ int u8p_rotation(int j, int tile, int n_img, int tiles_per_img, int nsteps) {
    const int full = (n_img / 8) * 8;
    const int old_wg8 = j < full ? (j >> 3) * tiles_per_img + tile : (j * tiles_per_img + tile) >> 3;
    return (int)((unsigned)old_wg8 % (unsigned)nsteps);
}

template <int PASSES, int NSTEPS>
__global__ __launch_bounds__(U8P_THREADS, 4) void conv_fwd_u8_pair_kernel(const ConvImgParams p) {
    ISDQN_EMPTY_KERNEL_RETURN
    constexpr int MT = 2, NT = 2, MTW = MT, NTHR = U8P_THREADS, STACK_MAX = 4;
    constexpr int W_PLANES = PASSES >= 2 ? 2 : 1;
    static_assert(NSTEPS * GEMM_BK == 256, "resident weights: [32][256 k]");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __bf16* smem = reinterpret_cast<__bf16*>(smem_raw);
    __bf16* w_hi = smem;               // [32][U8P_WPITCH]
    __bf16* w_lo = smem + U8P_WPLANE;  // (PASSES >= 2)
    __bf16* img = smem + W_PLANES * U8P_WPLANE;
    const ConvGeom& g = p.g;
    const int tid = threadIdx.x, lane = tid & 63, grp = lane >> 4;
    const int wave = (tid >> 6) & 3, hw = tid >> 8;  // wave inside its group of four / which tile of the half the group computes
#if defined(ISDQN_DEV)
#define U8P_STAMP(i)                                                                                 \
    if (p.stamps != nullptr && threadIdx.x == 0) {                                                  \
        p.stamps[(int64_t)blockIdx.x * 8 + (i)] = (long long)__builtin_amdgcn_s_memtime();           \
        if ((i) == 0) p.stamps[(int64_t)blockIdx.x * 8 + 7] = (long long)__builtin_amdgcn_s_memrealtime(); \
    }
#else
#define U8P_STAMP(i)
#endif
    U8P_STAMP(0);
    const int j = (int)blockIdx.x;           // image
    const int n_half = p.tiles_per_img >> 1;  // halves of two old tiles

    __shared__ __attribute__((aligned(16))) float s_par[3][64];
    float par_v = 0.f;
    {
        const int which = tid >> 6, ch = tid & 63;
        const float* src = which == 0 ? p.bias : which == 1 ? p.gamma : p.beta;
        const bool ok = tid < 192 && ch < g.cout_p && src != nullptr;
        ISDQN_BOUNDS_CHECK(ok ? src + ch : zero_chunk(), 4, 13);
        par_v = *(const ISDQN_GLOBAL float*)(ok ? src + ch : zero_chunk());
    }
    constexpr int nsteps = NSTEPS;  // K / 32 = 2 * stacked frames, a compile-time constant: the K loop is straight-line code
    const int k_last = g.K - 8;
    // The weights: chunk c = tid + i * 512 of the 32 x 32 chunks is row c / 32, k chunk c % 32 (a wave reads 2 KB of two rows and writes
    // them to LDS 16 contiguous bytes per lane).  Requested first: they need no frame id, so they travel under that round trip.
    float wv[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) p.W.load((tid >> 5) + i * 16, (tid & 31) * 8, wv[i]);

    // ---- frame rows of one half: request (registers only) / convert into the LDS image ----
    const FrameSrc& fs = p.fs;
    const uint8_t* base[STACK_MAX];
#pragma unroll
    for (int c = 0; c < STACK_MAX; ++c) {
        const int id = c < fs.stack ? fs.frame_id(j, c) : -1;
        base[c] = id >= 0 ? fs.frames + (int64_t)id * fs.stride : nullptr;
    }
    const uint8_t* zeros = reinterpret_cast<const uint8_t*>(zero_chunk());
    const int cpr = p.Wp / 8, plane = p.Rd * p.Wp;
    auto half_rows = [&](int h, int& row_base) {  // global input row of local row 0 of half h; returns the positions of one plane
        const int oy_min = (int)g.d_wout.div((uint32_t)(h * 256));
        const int oy_max = (int)g.d_wout.div((uint32_t)(min(g.npix, h * 256 + 256) - 1));
        row_base = oy_min * g.stride - g.pad;
        return ((oy_max - oy_min) * g.stride + g.ksz) * cpr;
    };
    typedef unsigned long long RawRows[U8P_PB][STACK_MAX];  // the only registers a request keeps alive (shift and LDS offset are recomputed)
    auto request = [&](RawRows& raw, int h) {  // loads only: nothing here touches the loaded registers (a half past the image: zeros)
        int row_base = 0;
        const int per_plane = h < n_half ? half_rows(h, row_base) : 0;
#pragma unroll
        for (int k = 0; k < U8P_PB; ++k) {
            const int pos = k * NTHR + tid;
            const bool on = pos < per_plane;
            uint32_t lr, cx;
            p.d_chunk.divmod((uint32_t)(on ? pos : 0), lr, cx);
            const int iy = row_base + (int)lr, ix0 = (int)cx * 8 - g.pad;
            const bool ok = on && iy >= 0 && iy < fs.H && ix0 > -8 && ix0 < fs.W;
            const int ixc = min(max(ix0, 0), fs.W - 8);
            const int off = iy * fs.W + ixc;
#pragma unroll
            for (int c = 0; c < STACK_MAX; ++c) raw[k][c] = load_u64_unaligned((ok && base[c] != nullptr) ? base[c] + off : zeros);
        }
    };
    auto commit = [&](const RawRows& raw, int h) {
        int row_base;
        const int per_plane = half_rows(h, row_base);
#pragma unroll
        for (int k = 0; k < U8P_PB; ++k) {
            const int pos = k * NTHR + tid;
            if (pos - lane >= per_plane) continue;  // (wave-uniform: none of this wave's 64 positions is in the image of the half)
            const bool on = pos < per_plane;
            uint32_t lr, cx;
            p.d_chunk.divmod((uint32_t)(on ? pos : 0), lr, cx);
            const int ix0 = (int)cx * 8 - g.pad;
            const int sh = ix0 - min(max(ix0, 0), fs.W - 8);
            const int dst = (int)lr * p.Wp + (int)cx * 8;
#pragma unroll
            for (int c = 0; c < STACK_MAX; ++c) {
                if (c >= fs.stack) continue;
                float v[8];
                FrameSrc::patch8_cvt(raw[k][c], sh, v);
                bf16x8 hi;
                round8(v, hi);
                if (on) *reinterpret_cast<bf16x8*>(img + c * plane + dst) = hi;
            }
        }
    };

    // ---- everything this image needs from global memory, back to back: (the weights,) half 0's rows, half 1's rows ----
    RawRows raw0, raw1;
    request(raw0, 0);
    request(raw1, 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // (the oldest loads: written to LDS while the rows travel)
        const int at = ((tid >> 5) + i * 16) * U8P_WPITCH + (tid & 31) * 8;
        bf16x8 hi, lo;
        if constexpr (PASSES >= 2) {
            s8_unpack(wv[i], hi, lo);
            *reinterpret_cast<bf16x8*>(w_lo + at) = lo;
        } else {
            s8_unpack_hi(wv[i], hi);
        }
        *reinterpret_cast<bf16x8*>(w_hi + at) = hi;
    }
    if (tid < 192) s_par[tid >> 6][tid & 63] = par_v;
    commit(raw0, 0);

    struct Frags {
        bf16x8 a_hi[MTW], a_lo[MTW], b_hi[NT];
    };

    // One half: this wave's 32 pixels of old tile 2h + hw.  No barrier inside: a wave without a live pixel leaves at once.
    auto do_half = [&](int h) {
        const int tile = 2 * h + hw;
        const int p0 = tile * 128;
        if (p0 + wave * 32 >= g.npix) return;  // (wave-uniform)
        int row_base;
        half_rows(h, row_base);
        const int rot = u8p_rotation(j, tile, p.n_img, p.tiles_per_img, nsteps);
        auto slice = [&](int s) {  // (s < nsteps wherever it is called)
            const int k = s + rot;
            return k >= nsteps ? k - nsteps : k;
        };

        int b_org[NT], out_pix[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            int pp = p0 + wave * 32 + nt * 16 + (lane & 15);
            const bool in_img = pp < g.npix;
            pp = in_img ? pp : g.npix - 1;
            uint32_t oy_u, ox_u;
            g.d_wout.divmod((uint32_t)pp, oy_u, ox_u);
            const int oy = (int)oy_u, ox = (int)ox_u;
            out_pix[nt] = in_img ? oy * g.wout + ox : -1;
            const int ly0 = oy * g.stride - g.pad - row_base;
            const int lx0 = ox * g.stride;
            b_org[nt] = ly0 * p.Wp + lx0;
        }
        f32x4 acc[MTW][NT];
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) mfma_init(acc[mt][nt]);

        auto read_frags = [&](int kk, Frags& f) {
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt) {
                f.a_hi[mt] = read_frag<false, U8P_WPITCH>(w_hi + kk * GEMM_BK, mt * 16, lane);
                if constexpr (PASSES >= 2) f.a_lo[mt] = read_frag<false, U8P_WPITCH>(w_lo + kk * GEMM_BK, mt * 16, lane);
            }
            int kq = kk * GEMM_BK + grp * 8;
            kq = kq < k_last ? kq : k_last;
            const int c = kq >> 6, ky = (kq >> 3) & 7;
            const int tap_off = (c * p.Rd + ky) * p.Wp;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const __bf16* src = img + b_org[nt] + tap_off;
                typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
                bf16x4 h0 = *reinterpret_cast<const bf16x4*>(src);
                bf16x4 h1 = *reinterpret_cast<const bf16x4*>(src + 4);
                f.b_hi[nt] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
            }
        };
        auto mfma_step = [&](const Frags& f) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) {
                    if constexpr (PASSES >= 2) mfma_acc(acc[mt][nt], f.a_lo[mt], f.b_hi[nt]);
                    mfma_acc(acc[mt][nt], f.a_hi[mt], f.b_hi[nt]);
                }
        };
        // conv_fwd_img_kernel's K walk, from LDS only: the fragments of step s + 1 are read under the MFMAs of step s
        Frags fr[2];
        read_frags(slice(0), fr[0]);
#pragma unroll
        for (int s = 0; s < NSTEPS; ++s) {
            if (s + 1 < NSTEPS) read_frags(slice(s + 1), fr[(s + 1) & 1]);
            mfma_step(fr[s & 1]);
            constexpr int N_MFMA = MTW * NT * PASSES;
#pragma unroll
            for (int i = 0; i < N_MFMA; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, PASSES >= 2 ? 1 : 2, 0);
            }
        }

        U8P_STAMP(h == 0 ? 2 : 5);  // K loop done
        // ---- epilogue: bias + LayerNorm over channels + ReLU (conv_fwd_img_kernel's, KG = 1) ----
        float bi[MTW][4], ga[MTW][4], be[MTW][4];
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
            const int ch0 = (mt * 16 + grp * 4) & 63;
            const float4 b4 = *reinterpret_cast<const float4*>(&s_par[0][ch0]);
            const float4 g4 = *reinterpret_cast<const float4*>(&s_par[1][ch0]);
            const float4 e4 = *reinterpret_cast<const float4*>(&s_par[2][ch0]);
            bi[mt][0] = b4.x; bi[mt][1] = b4.y; bi[mt][2] = b4.z; bi[mt][3] = b4.w;
            ga[mt][0] = g4.x; ga[mt][1] = g4.y; ga[mt][2] = g4.z; ga[mt][3] = g4.w;
            be[mt][0] = e4.x; be[mt][1] = e4.y; be[mt][2] = e4.z; be[mt][3] = e4.w;
        }
        const float inv_c = 1.0f / (float)g.cout;
        float zv[NT][MTW][4], s1[NT], s2[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            s1[nt] = s2[nt] = 0.f;
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int ch = mt * 16 + grp * 4 + r;
                    float zz = ch < g.cout ? acc[mt][nt][r] * p.scale + bi[mt][r] : 0.f;
                    zv[nt][mt][r] = zz;
                    s1[nt] += zz;
                    s2[nt] += zz * zz;
                }
            if (p.gamma != nullptr) {
                s1[nt] += __shfl_xor(s1[nt], 16); s1[nt] += __shfl_xor(s1[nt], 32);
                s2[nt] += __shfl_xor(s2[nt], 16); s2[nt] += __shfl_xor(s2[nt], 32);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float mean = 0.f, rstd = 1.f;
            if (p.gamma != nullptr) {
                mean = s1[nt] * inv_c;
                float var = fmaxf(s2[nt] * inv_c - mean * mean, 0.f);
                rstd = rsqrtf(var + 1e-6f);
            }
            if (out_pix[nt] >= 0) {
                const int64_t pix = (int64_t)j * g.npix + out_pix[nt];
                // the activations leave write-through (gemm_core.h): this image's rows are the buffer, the pixel's row the offset
                const int row_off = out_pix[nt] * g.cout_p * 4;
                const WriteThroughDst act_dst = write_through_dst(p.act + (int64_t)j * g.npix * g.cout_p, g.npix * g.cout_p * 4);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) {
                    int ch0 = mt * 16 + grp * 4;
                    if (ch0 >= g.cout_p) continue;
                    float4 a, zq;
                    float* ap = &a.x;
                    float* zp = &zq.x;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float y = p.gamma != nullptr ? (zv[nt][mt][r] - mean) * (rstd * ga[mt][r]) + be[mt][r] : zv[nt][mt][r];
                        ap[r] = (ch0 + r < g.cout) ? fmaxf(y, 0.f) : 0.f;
                        zp[r] = zv[nt][mt][r];
                    }
                    s8_store_quad_paired(act_dst, row_off, ch0, a.x, a.y, a.z, a.w);
                    // (a nontemporal store of z -- not read before the backward -- was measured: 26.5 -> 28.0 us)
                    if (j < p.z_img) *reinterpret_cast<float4*>(p.z + pix * g.cout_p + ch0) = zq;
                }
            }
        }
        U8P_STAMP(h == 0 ? 3 : 6);  // epilogue stores issued
    };

    U8P_STAMP(1);  // half 0's image and the weights written (this thread)
    for (int h = 0; h < n_half; ++h) {
        __syncthreads();  // the image of half h (h == 0: and the weights, the epilogue parameters) visible
        do_half(h);
        if (h + 1 < n_half) {
            __syncthreads();  // every wave is done with the LDS image: the next half's rows may overwrite it
            commit(raw1, h + 1);
            U8P_STAMP(4);  // next half's image written
            if (h + 2 < n_half) request(raw1, h + 2);  // (images of more than four tiles: under the next half's K loop)
        }
    }
#undef U8P_STAMP
}

// LDS bytes of the kernel above: resident weights + the image of a half (`Rd` rows of `Wp` columns, four planes)
template <int PASSES>
static inline int conv_u8_pair_lds(int Rd, int Wp) {
    return ((PASSES >= 2 ? 2 : 1) * U8P_WPLANE + 4 * Rd * Wp) * 2;
}
// input rows that two consecutive 128-pixel tiles need together (conv_img_geometry's R for 256 pixels)
static inline int conv_u8_pair_rows(const ConvGeom& g) {
    int rows = g.npix <= 256 ? g.hout : ((256 + g.wout - 2) / g.wout + 1);
    if (rows > g.hout) rows = g.hout;
    return g.stride * (rows - 1) + g.ksz;
}

template <int PASSES, int NSTEPS>
static int launch_conv_fwd_u8_pair(const ConvImgParams& p, hipStream_t st) {
    const int lds = conv_u8_pair_lds<PASSES>(p.Rd, p.Wp);
    static LdsConfigured configured;
    if (int rc = ensure_dynamic_lds(&conv_fwd_u8_pair_kernel<PASSES, NSTEPS>, lds, configured)) return rc;
    const int grid = p.n_img;
    ISDQN_REPORT_OCCUPANCY((&conv_fwd_u8_pair_kernel<PASSES, NSTEPS>), U8P_THREADS, lds, grid);
    hipLaunchKernelGGL((conv_fwd_u8_pair_kernel<PASSES, NSTEPS>), dim3(grid), dim3(U8P_THREADS), lds, st, p);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

}  // namespace isdqn
