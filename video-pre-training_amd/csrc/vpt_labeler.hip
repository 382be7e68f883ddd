// Video labelling with the inverse dynamics model (gfx950): the two small kernels between the IDM's kernels when a whole recording is
// labelled in overlapping windows (IDMEngine.forward_windows), so that neither the features nor the labels leave HBM.
//
//  vpt_gather_rows_kernel : y[i][:] = x[index[i]][:] for fp32 rows of D values (D % 4 == 0: 16-byte loads and stores, one per thread).  Used
//        twice: per-frame features ("slots", computed once per distinct frame and clipped temporal neighbourhood) -> the rows of every
//        window in front of the first transformer block, and window rows -> the one row that labels each frame in front of final_ln and
//        the heads.  Replaces the reference's host-side windowing of the pixels (run_inverse_dynamics_model.py:146-163: one
//        agent.predict_actions(frames) per batch of frames) -- here the window is a list of row indices, not a copy of 128 frames.
//        An index outside [0, rows_in) yields a row of zeros (never a read outside x).
//  vpt_idm_decode_kernel  : one thread per frame turns the IDM's log-probs (buttons [N][20][2], camera [N][2][n_bins]) into labels --
//        InverseActionPolicy.predict's deterministic sample (lib/policy.py:448-464 over lib/action_head.py:195-207: arg-max per group, FIRST
//        maximum as torch.argmax and vpt_logsoftmax_kernel keep it) and the sum of the chosen log-probs (lib/action_head.py:176-193; added
//        left to right in fp32, buttons first), then what IDMAgent._agent_action_to_env does on the host after `.cpu().numpy()`
//        (inverse_dynamics_model.py:61-72): CameraQuantizer.undiscretize of the camera bins (lib/actions.py:100-108, fp64), and the way back
//        into the policy's joint indices for training on the labels, CameraHierarchicalMapping.from_factored (lib/action_mapping.py:179-207).
//        The arithmetic of the last two is vpt_action_codec.h's, the copy the codec's own kernels run.  `null` marks the frames the
//        reference's loader drops (data_loader.py:48-128: no button pressed, camera at the centre bin in both axes).
#include "vpt_common.h"
#include "vpt_kernels.h"
#include "vpt_action_codec.h"

__global__ __launch_bounds__(256) void vpt_gather_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ index, float* __restrict__ y,
                                                              long rows_in, long n, int D4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;     // one 16-byte piece of one output row
  if (i >= n * D4) return;
  const long row = i / D4;
  const int c = (int)(i - row * D4);
  const long r = index[row];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (r >= 0 && r < rows_in) v = *((const f32x4*)x + r * D4 + c);
  *((f32x4*)y + i) = v;
}

__global__ __launch_bounds__(256) void vpt_idm_decode_kernel(const float* __restrict__ lp_buttons, const float* __restrict__ lp_camera,
                                                             long* __restrict__ buttons, long* __restrict__ camera, float* __restrict__ log_prob,
                                                             long* __restrict__ joint_buttons, long* __restrict__ joint_camera,
                                                             double* __restrict__ camera_deg, uint8_t* __restrict__ null_flag, long n, int n_bins,
                                                             double maxval, double binsize, double mu, int mu_law) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long b[N_BUTTONS];
  float lp = 0.f;
  bool any = false;
  const float* zb = lp_buttons + i * (2 * N_BUTTONS);
#pragma unroll
  for (int g = 0; g < N_BUTTONS; ++g) {
    const float v0 = zb[2 * g], v1 = zb[2 * g + 1];
    const bool on = v1 > v0;                    // a tie keeps the lower index
    b[g] = on ? 1 : 0;
    const float v = on ? v1 : v0;
    lp = (g == 0) ? v : lp + v;
    any |= on;
    buttons[i * N_BUTTONS + g] = b[g];
  }
  long cbin[2];
#pragma unroll
  for (int ax = 0; ax < 2; ++ax) {
    const float* zc = lp_camera + (i * 2 + ax) * n_bins;
    float best = zc[0];
    int besti = 0;
    for (int k = 1; k < n_bins; ++k) {
      const float v = zc[k];
      if (v > best) { best = v; besti = k; }    // ascending k: keeps the first maximum
    }
    cbin[ax] = besti;
    lp = lp + best;
    camera[i * 2 + ax] = besti;
    camera_deg[i * 2 + ax] = vpt_camera_undiscretize_one(besti, maxval, binsize, mu, mu_law);
  }
  log_prob[i] = lp;
  vpt_action_from_factored_one(b, cbin[0], cbin[1], n_bins, joint_buttons + i, joint_camera + i);
  const int null_bin = n_bins / 2;
  null_flag[i] = (!any && cbin[0] == null_bin && cbin[1] == null_bin) ? 1 : 0;
}

extern "C" int vpt_gather_rows_launch(const float* x, const int32_t* index, float* y, long rows_in, long n, int D, hipStream_t stream) {
  if (!x || !index || !y || rows_in <= 0 || n <= 0 || D <= 0 || (D & 3)) return -1;
  if (((uintptr_t)x | (uintptr_t)y) & 15) return -1;
  const long blocks = (n * (D >> 2) + 255) / 256;
  if (blocks > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(vpt_gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, index, y, rows_in, n, D >> 2);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int vpt_idm_decode_launch(const float* lp_buttons, const float* lp_camera, int64_t* buttons, int64_t* camera, float* log_prob,
                                     int64_t* joint_buttons, int64_t* joint_camera, double* camera_deg, uint8_t* null_flag, long n, int n_camera_bins,
                                     double maxval, double binsize, double mu, int mu_law, hipStream_t stream) {
  if (!lp_buttons || !lp_camera || !buttons || !camera || !log_prob || !joint_buttons || !joint_camera || !camera_deg || !null_flag) return -1;
  if (n <= 0 || n_camera_bins < 1 || !(n_camera_bins & 1) || maxval <= 0.0 || binsize <= 0.0 || (mu_law && mu <= 0.0)) return -1;
  const long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(vpt_idm_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, lp_buttons, lp_camera, (long*)buttons, (long*)camera, log_prob,
                     (long*)joint_buttons, (long*)joint_camera, camera_deg, null_flag, n, n_camera_bins, maxval, binsize, mu, mu_law);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
