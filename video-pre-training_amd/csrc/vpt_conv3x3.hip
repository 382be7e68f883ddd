// 3x3 / pad-1 convolution of the IMPALA residual CNN: the launch function -- argument validation, mode, tiling and halo-DMA selection.  The kernels live
// one family per source, each behind an internal launcher (vpt_kernels.h): vpt_conv3x3_fwd.hip (forward modes 0, 1, 4, 5, 7 + the pool seam pass),
// vpt_conv3x3_dgrad.hip (dgrad modes 2, 3, 6), vpt_conv3x3_small.hip (the latency tiling); what they share: vpt_conv3x3_tile.h.
#include "vpt_conv3x3_tile.h"
#include <stdlib.h>
static long long* g_conv_trace = nullptr;
extern "C" void vpt_conv3x3_set_trace(void* buf) { g_conv_trace = (long long*)buf; }  // profiling: [grid][12] int64, or null

// which forward modes take the halo-DMA instantiation where the shape allows it: bit 0 = modes 0, 1, 5; bit 1 = the pool-fused mode 4
#define HALO_DMA_DEFAULT 3
static int g_conv_halo_dma = HALO_DMA_DEFAULT;
// tests and A/B measurements: 0 = the register-staged path everywhere, a negative value = the shipped selection; returns the previous mask
extern "C" int vpt_conv3x3_set_halo_dma(int mask) { const int was = g_conv_halo_dma; g_conv_halo_dma = mask < 0 ? HALO_DMA_DEFAULT : (mask & 3); return was; }

extern "C" int vpt_conv3x3_launch(const VptConv3x3Args* a_in, hipStream_t stream) {
  int ablate = 0, extra_lds = 0;
#ifdef VPT_CONV_PROFILE
  static int ablate_env = -1, extra_lds_env = 0;
  if (ablate_env < 0) {
    const char* e = getenv("VPT_CONV_ABLATE");
    ablate_env = e ? atoi(e) : 0;
    const char* xl = getenv("VPT_CONV_EXTRA_LDS");  // dynamic LDS bytes (> 2 KB forces one workgroup per CU; the forward launcher raises the kernels' limit)
    extra_lds_env = xl ? atoi(xl) : 0;
  }
  ablate = ablate_env; extra_lds = extra_lds_env;
#endif
  VptConv3x3Args a_copy = *a_in;
  a_copy.ablate = ablate;
  a_copy.trace = g_conv_trace;
  const VptConv3x3Args* a = &a_copy;
  if ((a->H & 15) || (a->W & 15) || (a->Cin & 31) || (a->Cout & 31) || a->frames <= 0) return -1;
  const long grid = (long)a->frames * (a->H >> 4) * (a->W >> 4) * a->NT;
  if (grid > 0x7fffffffL) return -2;
  const int mode = a->bwd ? (a->res ? 3 : (a->gate_stats ? 6 : 2)) : (a->pool ? (a->pool_mask ? 7 : 4) : (a->res ? (a->res_bias ? 5 : 1) : 0));
  if (a->pool_mask && !a->pool) return -1;
  if (a->gate_stats && (!a->bwd || a->res || !a->gate_u || a->trace)) return -1;   // the gated dgrad: no skip connection (a block's conv1 -> conv0)
  if ((a->res_bias != nullptr) != (a->res_scale != nullptr) || (a->res_bias && (a->bwd || !a->res))) return -1;
  if ((a->kk_frame != nullptr) != (a->rs_frame != nullptr) || (a->kk_frame && a->bwd)) return -1;
  if (a->bwd && (!a->xin || !a->coef)) return -1;   // dgrad always carries the GroupNorm-statistics terms (c0 + c1 * xin)
  if (a->pool && (a->bwd || a->res || (a->tiling != 1 && a->tiling != 3) || a->trace || !a->seam_r || !a->seam_c)) return -1;
  // the latency tiling (32 output channels per workgroup) is the CALLER's choice, never the grid size's: a frame's result must not
  // depend on how many frames share the launch (the two tilings sum a tile's statistics in different orders)
  if (!a->bwd && a->tiling != 1 && a->tiling != 2 && a->tiling != 3) return -1;
  if (!a->bwd && !a->trace && a->tiling == 2) {
    const long sgrid = (long)a->frames * (a->H >> 4) * (a->W >> 4) * (a->Cout >> 5);
    vpt_conv3x3_small_launch(a, sgrid, stream);
    return hipGetLastError() == hipSuccess ? 0 : -3;
  }
  if (a->trace && mode > 3) return -1;
  if (mode == 6) { vpt_conv3x3_dgrad_launch(a, 6, grid, extra_lds, stream); return hipGetLastError() == hipSuccess ? 0 : -3; }
  // Halo DMA (HDMA): the 16-row forward modes on an even count of 32-channel blocks (a pass of its loop is two blocks) whose frame fits the
  // 2^30-byte offset range below H_OOB.  Everything else -- odd counts, tracing, profile builds with extra LDS -- runs the register-staged
  // instantiation, which is also the bitwise reference of tests/test_gpu_conv_halo_dma.py (vpt_conv3x3_set_halo_dma(0) sends every launch there).
  const bool hdma_shape = !a->bwd && !a->trace && !extra_lds && ((a->Cin >> 5) & 1) == 0 && (long long)(a->Cin >> 5) * a->H * a->W * 64 < (long long)H_OOB;
  // (mode 7, the pool-fused training forward with arg-max masks, lost 4 % on the K = 1152 layer under the new schedule and won 2.5 % on the K = 2304
  // one -- profiles/conv3x3_halo_dma.md -- so it keeps the register-staged instantiation)
  if (mode == 7) { vpt_conv3x3_fwd_launch(a, 7, 0, grid, extra_lds, stream); return hipGetLastError() == hipSuccess ? 0 : -3; }
  // tiling 3 (forward) = the 32-row, eight-wave tiles wherever the image has whole 32-row bands.  Measured at parity with the 16-row tiles on
  // every layer shape (profiles/r04_experiments.md section 7: halving the weight DMA buys nothing on a power-limited chip), so the shipped
  // choice stays the 16-row kernel; the variant is kept selectable because it is bit-identical per pixel and covered by the same tests.
  if (!a->trace && !a->bwd && mode != 4 && (a->H & 31) == 0 && a->tiling == 3 && !extra_lds) {
    const long g32 = grid >> 1;
    vpt_conv3x3_fwd_launch(a, mode, 1, g32, 0, stream);
    return hipGetLastError() == hipSuccess ? 0 : -3;
  }
  if (hdma_shape && (((g_conv_halo_dma & 1) && (mode == 0 || mode == 1 || mode == 5)) || ((g_conv_halo_dma & 2) && mode == 4))) {
    vpt_conv3x3_fwd_launch(a, mode, 2, grid, 0, stream);
    return hipGetLastError() == hipSuccess ? 0 : -3;
  }
  if (a->bwd) vpt_conv3x3_dgrad_launch(a, mode, grid, extra_lds, stream);
  else vpt_conv3x3_fwd_launch(a, mode, 0, grid, extra_lds, stream);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
