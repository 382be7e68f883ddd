// Temporal Conv3d of the inverse dynamics model fused with the uint8 ingest, bias and ReLU (gfx950), and its weight / bias gradient
// (vpt_conv3d_t5_bwd_kernel, further down).
//
// Replaces ImgPreprocessing.forward (x/255, lib/policy.py:39-45) + InverseActionNet._conv3d_forward
// (lib/policy.py:394-403): Conv3d(3 -> O, kernel (5,1,1), padding (2,0,0)) over the T axis of each sequence
// + ReLU (FanInInitReLULayer without norm, so with bias; lib/policy.py:366-372).
//
// out[b,t,h,w,o] = relu( sum_{dt=-2..2} sum_c W[o,c,dt] * img[b,t+dt,h,w,c] / 255 + bias[o] ), zero outside [0,T).
// K = 15 (padded to 16): one MFMA 32x32x16 k-step with swapped operands (weights = A rows, pixels = B
// columns; 0..255 are exact in bf16, 1/255 applied in fp32), so a lane owns one pixel and groups of 4
// consecutive output channels -> 8-byte stores into the channel-blocked layout [frame][O/32][H][W][32].
// One workgroup = 256 consecutive pixels of one frame x 128 output channels; the five input frames' bytes
// (5 x 768 B) are staged in LDS with 16-byte loads.  Emits sum / sum-of-squares per frame for the GroupNorm
// of the following stack-0 firstconv (first_conv_norm=True in the IDM, lib/policy.py:360-363).
#include "vpt_common.h"
#include "vpt_kernels.h"

// INDEXED (vpt_conv3d_t5_forward_indexed, the video labeller's shared-feature path): output frame j ("slot") is centred on img[src[j]] and
// tap dt reads img[src[j] + dt - 2] iff lo[j] <= src[j] + dt - 2 < hi[j] -- the zero padding of whichever window the slot stands for, without
// a copy of that window's pixels.  The plain kernel is the case src[j] = j, [lo, hi) = the frame's own sequence; both run this one body.
template <bool INDEXED>
__device__ __forceinline__ void vpt_conv3d_t5_body(const VptConv3dArgs& a) {
  __shared__ __attribute__((aligned(16))) unsigned char in[5 * 768];
  __shared__ __attribute__((aligned(16))) float bias_s[128];
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int HW = a.H * a.W;
  const int chunks = HW >> 8;  // 256-pixel chunks per frame
  int L = blockIdx.x;
  const int nt = L % a.NT; L /= a.NT;
  const int chunk = L % chunks;
  const int f = L / chunks;       // output frame: b*T + t, or the slot
  const int p0 = chunk * 256;
  int fc, f_lo, f_hi;             // centre frame in img and the range of img frames its taps may read
  if constexpr (INDEXED) {
    fc = a.src[f];
    f_lo = max(a.lo[f], 0);       // (never outside img, whatever the plan says)
    f_hi = min(a.hi[f], a.n_img);
  } else {
    fc = f;
    f_lo = f - f % a.T;
    f_hi = f_lo + a.T;
  }

  if (tid < 240) {
    const int dt = tid / 48, c16 = tid - dt * 48;  // 48 x 16 B = 768 B per frame slab
    const int ft = fc + dt - 2;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ft >= f_lo && ft < f_hi) v = *(const u32x4*)(a.img + ((size_t)ft * HW + p0) * 3 + c16 * 16);
    *(u32x4*)(in + dt * 768 + c16 * 16) = v;
  }
  if (tid < 128) bias_s[tid] = a.bias[nt * 128 + tid];
  op16x8 wfr[4];
#pragma unroll
  for (int cs = 0; cs < 4; ++cs) wfr[cs] = *((const op16x8*)a.wfrag + (nt * 4 + cs) * 64 + lane);
  __syncthreads();

  const int CB_out = a.Cout >> 5;
  float s_sum = 0.f, s_sq = 0.f;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    const int pl = w * 64 + sub * 32 + l31;  // pixel within the chunk
    float h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kA = e, kB = 8 + e;  // k for lanes 0-31 / 32-63; k = dt*3 + ch, k = 15 is padding
      const int offA = (kA / 3) * 768 + (kA % 3), offB = (kB < 15) ? (kB / 3) * 768 + (kB % 3) : 0;
      float v = (float)in[pl * 3 + (hi ? offB : offA)];   // a byte: exact in either 16-bit operand format
      if (kB >= 15) v = hi ? 0.f : v;
      h[e] = v;
    }
    const u32x4 pk = {pack_op16x2_exact(h[0], h[1]), pack_op16x2_exact(h[2], h[3]), pack_op16x2_exact(h[4], h[5]), pack_op16x2_exact(h[6], h[7])};
    const op16x8 pf = __builtin_bit_cast(op16x8, pk);
    const size_t pbase = ((size_t)f * CB_out + nt * 4) * HW * 32 + (size_t)(p0 + pl) * 32 + 4 * hi;
#pragma unroll
    for (int cs = 0; cs < 4; ++cs) {
      if (nt * 4 + cs >= CB_out) continue;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      acc = VPT_MFMA_32X32X16(wfr[cs], pf, acc, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = *(const f32x4*)(bias_s + cs * 32 + 8 * g + 4 * hi);
        const float v0 = fmaxf(fmaf(acc[4 * g + 0], 1.0f / 255.0f, b4.x), 0.f);
        const float v1 = fmaxf(fmaf(acc[4 * g + 1], 1.0f / 255.0f, b4.y), 0.f);
        const float v2 = fmaxf(fmaf(acc[4 * g + 2], 1.0f / 255.0f, b4.z), 0.f);
        const float v3 = fmaxf(fmaf(acc[4 * g + 3], 1.0f / 255.0f, b4.w), 0.f);
        s_sum += (v0 + v1) + (v2 + v3);
        s_sq = fmaf(v0, v0, fmaf(v1, v1, fmaf(v2, v2, fmaf(v3, v3, s_sq))));
        const u32x2 o = {pack_op16x2(v0, v1), pack_op16x2(v2, v3)};
        *(u32x2*)(a.y + pbase + (size_t)cs * HW * 32 + 8 * g) = o;
      }
    }
  }
  if (a.stats_out) {
    s_sum = wave_sum(s_sum);
    s_sq = wave_sum(s_sq);
    if (lane == 0) { red[w] = s_sum; red[4 + w] = s_sq; }
    __syncthreads();
    if (tid == 0) {
      atomicAdd(a.stats_out + 2 * f, (double)((red[0] + red[1]) + (red[2] + red[3])));
      atomicAdd(a.stats_out + 2 * f + 1, (double)((red[4] + red[5]) + (red[6] + red[7])));
    }
  }
}

__global__ __launch_bounds__(256, 2) void vpt_conv3d_t5_kernel(VptConv3dArgs a) { vpt_conv3d_t5_body<false>(a); }
__global__ __launch_bounds__(256, 2) void vpt_conv3d_t5_indexed_kernel(VptConv3dArgs a) { vpt_conv3d_t5_body<true>(a); }

extern "C" int vpt_conv3d_launch(const VptConv3dArgs* a, hipStream_t stream) {
  if (((a->H * a->W) & 255) || (a->Cout & 31) || a->frames <= 0 || a->T <= 0 || (a->frames % a->T)) return -1;
  const long grid = (long)a->frames * ((a->H * a->W) >> 8) * a->NT;
  if (grid > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(vpt_conv3d_t5_kernel, dim3((unsigned)grid), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------------------------------------
// Backward of the temporal conv w.r.t. its weight and bias (the input is the uint8 image: no dgrad).  With g = dy * [y > 0], the gate read from the
// STORED forward output as every other backward kernel does:
//     dW[o][c][dt] = (1/255) sum_{f,p} g[f][p][o] * img[f + dt - 2][p][c]   (tap inside frame f's own sequence, else 0),   db[o] = sum_{f,p} g[f][p][o].
// The forward's mapping transposed: the reduction axis of the MFMA 32x32x16 is PIXELS.  A = g^T (rows = the 32 channels of the wave's block; g lies
// channel-fastest in HBM, so the wave stages 64 pixels x 64 B in LDS exactly as they lie there and ds_read_b64_tr_b16 hands every lane 8 pixels of
// its channel, as in vpt_conv_wgrad_kernel), B = the 15 taps of the same pixels as exact 16-bit bytes (columns k = dt*3 + ch), column 15 a constant 1
// so that db falls out of the same MFMA; columns 16..31 are zero (half the matrix pipe idles: the kernel is bound by the 512 B / pixel of y and dy).
// The products are exact in fp32 (8-bit x <= 11-bit significands), only the summation order rounds.
// Workgroup = 4 waves = the 4 channel blocks of up to 128 channels, sweeping a contiguous range of (frame, 256-pixel chunk) items with the accumulators
// in registers; the five 768-byte image slabs of an item are shared by the waves and double-buffered (one barrier per item), the g tile is private to
// its wave (LDS operations of one wave execute in order: no barrier between its stores and its transpose reads).  Every workgroup writes one slab row
// [Cout*15 | Cout] and vpt_slab_sum adds the rows in a fixed order: no float atomics, the same inputs give the same bits.
#define C3B_MAX_WG 512
__device__ __forceinline__ op16x8 tr_frag16(const unsigned char* p) {  // 8 pixels of this lane's channel: two 4-pixel transposes
  const op16x4 lo = lds_tr16_read(p);
  const op16x4 up = lds_tr16_read(p + 256);
  return __builtin_shufflevector(lo, up, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256, 2) void vpt_conv3d_t5_bwd_kernel(VptConv3dBwdArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char in[2][5 * 768];
  __shared__ __attribute__((aligned(16))) unsigned char gt[4][64 * 64];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, n = lane & 31;
  const int HW = a.H * a.W, chunks = HW >> 8, CB = a.Cout >> 5;
  const int items = a.frames * chunks;
  const int i0 = blockIdx.x * a.items_per_wg, i1 = min(i0 + a.items_per_wg, items);
  const bool active = w < CB;

  auto load_bytes = [&](int item) -> u32x4 {      // thread tid < 240: 16 bytes of tap frame tid / 48
    const int f = item / chunks, p0 = (item - f * chunks) * 256;
    const int dt = tid / 48, c16 = tid - dt * 48;
    const int f_lo = f - f % a.T, ft = f + dt - 2;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (tid < 240 && ft >= f_lo && ft < f_lo + a.T) v = *(const u32x4*)(a.img + ((size_t)ft * HW + p0) * 3 + c16 * 16);
    return v;
  };
  auto store_bytes = [&](int buf, const u32x4& v) {
    if (tid < 240) *(u32x4*)(in[buf] + tid * 16) = v;      // (dt * 768 + c16 * 16 == tid * 16)
  };
  u32x4 rd[4], ry[4];                             // 64 pixels x 64 B of dy and y of this wave's channel block: lane = (pixel j*16 + lane/4, 16-byte part lane%4)
  auto load_g = [&](int step) {
    const int item = step >> 2, sub = step & 3;
    const int f = item / chunks, p0 = (item - f * chunks) * 256 + sub * 64;
    const size_t base = ((size_t)(f * CB + w) * HW + p0 + (lane >> 2)) * 32 + (lane & 3) * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rd[j] = VPT_LD_STREAM((const u32x4*)(a.dy + base + j * 16 * 32));
      ry[j] = VPT_LD_STREAM((const u32x4*)(a.y + base + j * 16 * 32));
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int boff = (n < 15) ? (n / 3) * 768 + (n % 3) : 0;      // this lane's tap column in the byte slabs
  const int g16 = lane >> 4, i16 = lane & 15;
  const int lane_off = (8 * (g16 >> 1) + (i16 >> 2)) * 64 + (16 * (g16 & 1) + 4 * (i16 & 3)) * 2;   // vpt_conv_wgrad_kernel's fragment address
  unsigned char* tile = gt[w];

  u32x4 rb = {0u, 0u, 0u, 0u};
  if (i0 < i1) {
    rb = load_bytes(i0);
    store_bytes(0, rb);
    if (active) load_g(i0 * 4);
  }
  for (int item = i0; item < i1; ++item) {
    __syncthreads();                              // this item's bytes are visible; the other buffer's readers (the previous item) are done
    const int b = (item - i0) & 1;
    if (item + 1 < i1) rb = load_bytes(item + 1);
    if (active) {
      for (int sub = 0; sub < 4; ++sub) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {             // g = dy [y > 0] on the bit patterns (a positive 16-bit float is a positive signed integer)
          u32x4 g;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t yw = ry[j][q];
            const bool o0 = (short)(yw & 0xffffu) > 0, o1 = (short)(yw >> 16) > 0;
            g[q] = rd[j][q] & ((o0 ? 0xffffu : 0u) | (o1 ? 0xffff0000u : 0u));
          }
          *(u32x4*)(tile + (j * 16 + (lane >> 2)) * 64 + (lane & 3) * 16) = g;
        }
        load_g(min(item * 4 + sub + 1, i1 * 4 - 1));      // next step's loads fly during the MFMAs (the last step re-reads itself)
        const unsigned char* inb = in[b] + boff + (sub * 64 + 8 * hi) * 3;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const op16x8 af = tr_frag16(tile + ks * 16 * 64 + lane_off);
          float h[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = (float)inb[(ks * 16 + e) * 3];      // a byte: exact in either 16-bit operand format
            h[e] = (n < 15) ? v : ((n == 15) ? 1.f : 0.f);
          }
          const u32x4 pk = {pack_op16x2_exact(h[0], h[1]), pack_op16x2_exact(h[2], h[3]), pack_op16x2_exact(h[4], h[5]), pack_op16x2_exact(h[6], h[7])};
          acc = VPT_MFMA_32X32X16(af, __builtin_bit_cast(op16x8, pk), acc, 0, 0, 0);
        }
      }
    }
    if (item + 1 < i1) store_bytes(b ^ 1, rb);
  }

  // acc[r]: channel (r & 3) + 8 (r >> 2) + 4 hi of the wave's block, column n -> this workgroup's slab row, dW already in [o][c][dt] order
  if (active && n < 16) {
    float* row = a.partials + (size_t)blockIdx.x * (a.Cout * 16);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = w * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (n < 15) row[o * 15 + (n % 3) * 5 + n / 3] = acc[r] * (1.0f / 255.0f);
      else row[a.Cout * 15 + o] = acc[r];
    }
  }
}

static int conv3d_bwd_items_per_wg(long items) { return (int)((items + C3B_MAX_WG - 1) / C3B_MAX_WG); }

extern "C" long vpt_conv3d_bwd_partial_floats(int frames, int H, int W, int Cout) {
  const long items = (long)frames * (((long)H * W) >> 8);
  if (items <= 0) return 0;
  const int per = conv3d_bwd_items_per_wg(items);
  const int rows = (int)((items + per - 1) / per);
  return (long)rows * Cout * 16 + vpt_slab_sum_scratch_floats(rows, Cout * 16);
}

extern "C" int vpt_conv3d_bwd_launch(const VptConv3dBwdArgs* a_in, hipStream_t stream) {
  VptConv3dBwdArgs a = *a_in;
  if (((a.H * a.W) & 255) || (a.Cout & 31) || a.Cout <= 0 || a.Cout > 128 || a.frames <= 0 || a.T <= 0 || (a.frames % a.T)) return -1;
  if (!a.img || !a.y || !a.dy || !a.dw || !a.db || !a.partials) return -1;
  const long items = (long)a.frames * ((a.H * a.W) >> 8);
  if (items * 4 > 0x7fffffffL) return -2;
  a.items_per_wg = conv3d_bwd_items_per_wg(items);
  const int rows = (int)((items + a.items_per_wg - 1) / a.items_per_wg);
  hipLaunchKernelGGL(vpt_conv3d_t5_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -3;
  const int cols = a.Cout * 16;
  return vpt_slab_sum_launch(a.partials, rows, cols, cols, a.dw, a.Cout * 15, a.db, a.accumulate, a.partials + (size_t)rows * cols, stream);
}

// a->frames = number of slots (frames of y / stats_out), a->n_img = frames of img; a->T is not used
extern "C" int vpt_conv3d_indexed_launch(const VptConv3dArgs* a, hipStream_t stream) {
  if (((a->H * a->W) & 255) || (a->Cout & 31) || a->frames <= 0 || a->n_img <= 0 || !a->src || !a->lo || !a->hi) return -1;
  const long grid = (long)a->frames * ((a->H * a->W) >> 8) * a->NT;
  if (grid > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(vpt_conv3d_t5_indexed_kernel, dim3((unsigned)grid), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
