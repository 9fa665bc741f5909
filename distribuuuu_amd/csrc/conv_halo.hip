// Halo-staged 3x3 conv: bf16 NHWC, stride 1, pad 1, C=64 -> K=64.
//
// conv_smallk_pipe_kernel (conv.hip) feeds every MFMA of this shape from
// global loads: each input pixel is fetched nine times and the 72 KiB weight
// is re-read from L2 on every k-step. Here a persistent block keeps the
// whole weight in LDS, stages the input rows of one 256-pixel tile (halo
// included) into LDS once, and reads all nine taps from there.
//
// Same tile (256 consecutive m-rows), same wave ownership (64 rows x 64
// channels per wave), same MFMA instruction and the same (r, s, c) k-step
// order as conv_smallk_pipe_kernel, so y and the BN partials are
// bit-identical to it for any input.
//
// LDS image of the input: "padded rows" of W+1 pixels. Row index
// pr = n*(H+1) + h + 1; row n*(H+1) is the zero row shared by image n-1's
// bottom pad and image n's top pad, and column 0 of a row is the zero pixel
// shared by that row's left pad and the previous row's right pad. Pad pixels
// are written as zeros on every tile (never left over from an earlier tile:
// Inf * stale-bytes would poison the sum). Output pixel (n, h, w), tap (r, s)
// reads pixel index (pr - pr0 - 1 + r)*(W+1) + w + s.
//
// Both LDS images are XOR-swizzled at 16-byte granularity
// (chunk ^= (row >> 1) & 7, row = pixel resp. output channel) so a
// ds_read_b128 lane group, 16 different rows at one k-offset, spreads over
// the 16 slots of the 256-byte bank row.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int HALO_RSC = 576;                    // 3*3*64
constexpr int HALO_WROW_BYTES = HALO_RSC * 2;    // 1152 = 9 * 128
constexpr int HALO_W_BYTES = 64 * HALO_WROW_BYTES;
constexpr int HALO_SLAB_OFF = HALO_W_BYTES;      // 4 waves x [16][68] fp32
constexpr int HALO_XAREA_OFF = HALO_SLAB_OFF + 4 * 16 * 68 * 4;
constexpr int HALO_X_OFF = HALO_XAREA_OFF + 3 * 2 * 64 * 4;
constexpr int HALO_LDS_BYTES = 160 * 1024;
constexpr int HALO_MAX_PIX = (HALO_LDS_BYTES - HALO_X_OFF) / 128;  // 556
// 256 threads stage 32 pixels (8 x 16 B each) per pass
constexpr int HALO_STAGE_ITERS = (HALO_MAX_PIX + 31) / 32;

struct HaloConvParams {
  const __hip_bfloat16* x;
  const __hip_bfloat16* w;     // [64][3][3][64]
  __hip_bfloat16* y;
  const __hip_bfloat16* zbuf;  // 16 zero bytes
  float* part;                 // EMIT: [ceil(M/256), 128] BN partials
  int N, H, W, HW, M;
  int tq, trem;                // block b owns tq (+1 if b < trem) tiles
  unsigned long long magicHW, magicW, magicWp1, magicHp1;
};

DEV_INLINE int magic_div2(int m, unsigned long long magic) {
  return (int)(((unsigned long long)(unsigned)m * magic) >> 47);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void conv3x3_halo_kernel(HaloConvParams p) {
  __shared__ __align__(16) unsigned char smem[HALO_LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int Wp1 = p.W + 1, Hp1 = p.H + 1;
  const int b = blockIdx.x;
  int t = b * p.tq + min(b, p.trem);
  const int tend = t + p.tq + (b < p.trem ? 1 : 0);

  // padded-row index of output pixel m; wcol = its column
  auto prow_of = [&](int m, int& wcol) __attribute__((always_inline)) {
    const int n = magic_div2(m, p.magicHW);
    const int rem = m - n * p.HW;
    const int h = magic_div2(rem, p.magicW);
    wcol = rem - h * p.W;
    return n * Hp1 + h + 1;
  };
  // first padded row the tile's LDS image holds (one above its first pixel)
  auto tile_pr0 = [&](int tile) __attribute__((always_inline)) {
    int wc;
    return prow_of(tile * 256, wc) - 1;
  };

  // global -> registers: the tile's padded rows, zeros where the image ends.
  // Returns the number of LDS pixels the tile uses.
  const int spix = tid >> 3, sch = tid & 7;
  u32x4 stg[HALO_STAGE_ITERS];
  auto stage_load = [&](int tile) __attribute__((always_inline)) {
    int wc;
    const int pr0 = tile_pr0(tile);
    const int mlast = min(tile * 256 + 255, p.M - 1);
    const int nrows = prow_of(mlast, wc) + 2 - pr0;
    const int np = min(nrows * Wp1 + 1, HALO_MAX_PIX);
#pragma unroll
    for (int i = 0; i < HALO_STAGE_ITERS; ++i) {
      const int pix = spix + i * 32;
      const int prl = magic_div2(pix, p.magicWp1);
      const int col = pix - prl * Wp1;
      const int pr = pr0 + prl;
      const int n = magic_div2(pr, p.magicHp1);
      const int hh = pr - n * Hp1;
      const bool ok = pix < np && col >= 1 && hh >= 1 && n < p.N;
      const __hip_bfloat16* src =
          ok ? p.x + (((int64_t)n * p.H + (hh - 1)) * p.W + (col - 1)) * 64 +
                   sch * 8
             : p.zbuf;
      stg[i] = *reinterpret_cast<const u32x4*>(src);
    }
    return np;
  };
  auto stage_store = [&](int np) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < HALO_STAGE_ITERS; ++i) {
      const int pix = spix + i * 32;
      if (pix < np)
        *reinterpret_cast<u32x4*>(smem + HALO_X_OFF + pix * 128 +
                                  ((sch ^ ((pix >> 1) & 7)) << 4)) = stg[i];
    }
  };

  int np = stage_load(t);
  // weight -> LDS, once per block: 64 rows x 72 chunks of 16 B
#pragma unroll
  for (int i = 0; i < 64 * 72 / 256; ++i) {
    const int j = tid + i * 256;
    const int k = j / 72;
    const int ch = j - k * 72;
    const uint4 v = *reinterpret_cast<const uint4*>(p.w + (int64_t)j * 8);
    *reinterpret_cast<uint4*>(
        smem + k * HALO_WROW_BYTES +
        (((ch & ~7) | ((ch & 7) ^ ((k >> 1) & 7))) << 4)) = v;
  }
  stage_store(np);
  __syncthreads();

  // B-fragment byte offsets: output channel ni*16+il, k-offset kq*8 (+32 for
  // the second half of a tap: chunk bit 2, i.e. byte bit 6)
  int wb0[4], wb1[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    wb0[ni] = (ni * 16 + il) * HALO_WROW_BYTES + ((kq ^ (il >> 1)) << 4);
    wb1[ni] = wb0[ni] ^ 64;
  }

  for (; t < tend; ++t) {
    const bool more = t + 1 < tend;
    int npn = 0;
    if (more) npn = stage_load(t + 1);  // in flight under this tile's MFMAs

    const int m0 = t * 256;
    const int pr0 = tile_pr0(t);
    int abase[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = m0 + wid * 64 + mi * 16 + il;
      int wc;
      // rows past M compute on the tile's first pixel and are never stored
      const int pr = prow_of(m < p.M ? m : m0, wc);
      abase[mi] = (pr - pr0 - 1) * Wp1 + wc;
    }

    bf16x8 Af[2][4], Bf[2][4];
    // tap = r*3 + s, toff = r*(W+1) + s; the two 32-channel halves of a tap
    // use fragment buffers 0 and 1
    auto issue0 = [&](int tap, int toff) __attribute__((always_inline)) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int P = abase[mi] + toff;
        Af[0][mi] = *reinterpret_cast<const bf16x8*>(
            smem + HALO_X_OFF + P * 128 + ((kq ^ ((P >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        Bf[0][ni] =
            *reinterpret_cast<const bf16x8*>(smem + wb0[ni] + tap * 128);
    };
    auto issue1 = [&](int tap, int toff) __attribute__((always_inline)) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int P = abase[mi] + toff;
        Af[1][mi] = *reinterpret_cast<const bf16x8*>(
            smem + HALO_X_OFF + P * 128 + (((4 + kq) ^ ((P >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        Bf[1][ni] =
            *reinterpret_cast<const bf16x8*>(smem + wb1[ni] + tap * 128);
    };

    // One wave per SIMD: nothing else hides LDS latency, so each k-step's
    // eight reads must be issued a whole k-step (16 MFMAs) ahead of their
    // use. The scheduling barriers keep the compiler from sinking the reads
    // down to the MFMAs that consume them.
    f32x4 acc[4][4] = {};
    issue0(0, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      issue1(tap, (tap / 3) * Wp1 + tap % 3);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              Af[0][mi], Bf[0][ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (tap + 1 < 9)
        issue0(tap + 1, ((tap + 1) / 3) * Wp1 + (tap + 1) % 3);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              Af[1][mi], Bf[1][ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // epilogue: conv_smallk_pipe_kernel's, stripe for stripe
    float* slab = reinterpret_cast<float*>(smem + HALO_SLAB_OFF) + wid * 16 * 68;
    const int64_t mbase = (int64_t)m0 + wid * 64;
    const int er = lane >> 2, ec = (lane & 3) << 4;
    float ps = 0.f, pq = 0.f;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          slab[(kq * 4 + rr) * 68 + ni * 16 + il] = acc[mi][ni][rr];
      __builtin_amdgcn_wave_barrier();
      const int64_t m = mbase + mi * 16 + er;
      if (m < p.M) {
        union {
          __hip_bfloat16 b[16];
          uint4 q[2];
        } u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          u.b[j] = from_f32<__hip_bfloat16>(slab[er * 68 + ec + j]);
        __hip_bfloat16* yp = p.y + m * 64 + ec;
        *reinterpret_cast<uint4*>(yp) = u.q[0];
        *reinterpret_cast<uint4*>(yp + 8) = u.q[1];
      }
      if (EMIT)
        bn_partial_col_accum(
            slab, ps, pq,
            (int)min((int64_t)16, (int64_t)p.M - (mbase + mi * 16)), lane);
      __builtin_amdgcn_wave_barrier();
    }
    float(*xarea)[2][64] =
        reinterpret_cast<float(*)[2][64]>(smem + HALO_XAREA_OFF);
    if (EMIT && wid > 0) {
      xarea[wid - 1][0][lane] = ps;
      xarea[wid - 1][1][lane] = pq;
    }
    // every wave is past its last read of this tile's input image
    __syncthreads();
    if (EMIT && wid == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        ps += xarea[j][0][lane];
        pq += xarea[j][1][lane];
      }
      bn_partial_store(p.part, (int64_t)t * 128, 64, lane, 64, ps, pq);
    }
    if (more) stage_store(npn);
    __syncthreads();
  }
}

// LDS pixels the worst-placed tile of an [N, H, W] image batch needs
int64_t halo_pixels_needed(int64_t N, int64_t H, int64_t W) {
  const int64_t M = N * H * W;
  const int64_t T = std::min<int64_t>(256, M);
  const int64_t rows = std::min((T + W - 2) / W + 1, N * H);
  const int64_t imgs = std::min((T + H * W - 2) / (H * W) + 1, N);
  // image rows + one shared zero row per image touched + one more
  return (rows + imgs + 1) * (W + 1) + 1;
}

}  // namespace

// Geometry gate of the halo kernel (bf16 / 3x3 / stride 1 / pad 1 / 64->64 is
// the caller's to check): the tile's input image has to fit the LDS left
// beside the weight, and the magic divisions have to stay exact.
bool conv3x3_halo_admits(int64_t N, int64_t H, int64_t W) {
  if (N < 1 || H < 1 || W < 1 || N >= 65536 || H >= 65536) return false;
  const int64_t M = N * H * W;
  if (M >= (1LL << 31) || M * (H * W + 1) >= (1LL << 46) ||
      N * (H + 1) * (H + 1) >= (1LL << 46))
    return false;
  return halo_pixels_needed(N, H, W) <= HALO_MAX_PIX;
}

// Launch on the current stream. part == nullptr: no BN partials.
void conv3x3_halo_launch(const at::Tensor& x, const at::Tensor& w,
                         at::Tensor& y, const at::Tensor& zbuf, float* part) {
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3);
  TORCH_CHECK(conv3x3_halo_admits(N, H, W),
              "conv3x3_halo: geometry outside the LDS budget");
  HaloConvParams p;
  p.x = (const __hip_bfloat16*)x.data_ptr();
  p.w = (const __hip_bfloat16*)w.data_ptr();
  p.y = (__hip_bfloat16*)y.data_ptr();
  p.zbuf = (const __hip_bfloat16*)zbuf.data_ptr();
  p.part = part;
  p.N = (int)N; p.H = (int)H; p.W = (int)W;
  p.HW = (int)(H * W);
  p.M = (int)(N * H * W);
  p.magicHW = ((1ULL << 47) / (unsigned long long)(H * W)) + 1;
  p.magicW = ((1ULL << 47) / (unsigned long long)W) + 1;
  p.magicWp1 = ((1ULL << 47) / (unsigned long long)(W + 1)) + 1;
  p.magicHp1 = ((1ULL << 47) / (unsigned long long)(H + 1)) + 1;
  const int tiles = (p.M + 255) / 256;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int grid = std::min(tiles, std::max(cus, 1));
  p.tq = tiles / grid;
  p.trem = tiles % grid;
  if (part != nullptr)
    hipLaunchKernelGGL(conv3x3_halo_kernel<true>, dim3(grid), dim3(256), 0,
                       cur_stream(), p);
  else
    hipLaunchKernelGGL(conv3x3_halo_kernel<false>, dim3(grid), dim3(256), 0,
                       cur_stream(), p);
}
