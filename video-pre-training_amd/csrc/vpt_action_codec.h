// Per-row device functions of the action codec (gfx950), shared by the codec's own kernels (vpt_action_codec.hip) and the IDM
// label decoder (vpt_labeler.hip): ONE copy of the arithmetic of lib/actions.py:100-108 and lib/action_mapping.py:66-104, :179-207.
// Button order = Buttons.ALL (lib/actions.py:21-33): attack, back, forward, jump, left, right, sneak, sprint, use,
// drop, inventory, hotbar.1 .. hotbar.9.
#pragma once
#include "vpt_common.h"

#define B_ATTACK 0
#define B_BACK 1
#define B_FORWARD 2
#define B_JUMP 3
#define B_LEFT 4
#define B_RIGHT 5
#define B_SNEAK 6
#define B_SPRINT 7
#define B_USE 8
#define B_DROP 9
#define B_INVENTORY 10
#define B_HOTBAR1 11
#define N_BUTTONS 20
#define JOINT_INVENTORY 8640

// CameraQuantizer.undiscretize (lib/actions.py:100-108) of one bin, fp64.
__device__ __forceinline__ double vpt_camera_undiscretize_one(long bin, double maxval, double binsize, double mu, int mu_law) {
  double v = (double)bin * binsize - maxval;
  if (mu_law) {
    v = v / maxval;
    const double s = (v > 0.0) ? 1.0 : ((v < 0.0) ? -1.0 : 0.0);
    v = s * (1.0 / mu) * (pow(1.0 + mu, fabs(v)) - 1.0);
    v *= maxval;
  }
  return v;
}

// CameraHierarchicalMapping.from_factored (lib/action_mapping.py:179-207) of one row: b = its 20 button flags, (c0, c1) its camera bins.
__device__ __forceinline__ void vpt_action_from_factored_one(const long* b, long c0, long c1, int n_camera_bins, long* joint_buttons, long* joint_camera) {
  const int null_bin = n_camera_bins / 2;
  int hotbar = 0;
#pragma unroll
  for (int k = 1; k <= 9; ++k)
    if (b[B_HOTBAR1 + k - 1] != 0) hotbar = k;                       // later button wins
  const bool fwd = b[B_FORWARD] != 0, back = b[B_BACK] != 0;
  const int fore_back = (fwd && back) ? 0 : (back ? 2 : (fwd ? 1 : 0)); // both pressed cancel
  const bool left = b[B_LEFT] != 0, right = b[B_RIGHT] != 0;
  const int left_right = (left && right) ? 0 : (right ? 2 : (left ? 1 : 0));
  const int sprint_sneak = (b[B_SNEAK] != 0) ? 2 : ((b[B_SPRINT] != 0) ? 1 : 0);   // sneak is later in the group
  const int camera_on = !(c0 == null_bin && c1 == null_bin);
  long jb = hotbar;
  jb = jb * 3 + fore_back;
  jb = jb * 3 + left_right;
  jb = jb * 3 + sprint_sneak;
  jb = jb * 2 + (b[B_USE] != 0);
  jb = jb * 2 + (b[B_DROP] != 0);
  jb = jb * 2 + (b[B_ATTACK] != 0);
  jb = jb * 2 + (b[B_JUMP] != 0);
  jb = jb * 2 + camera_on;
  long jc = c0 * n_camera_bins + c1;
  if (b[B_INVENTORY] == 1) {                                           // exclusive with everything, camera included
    jb = JOINT_INVENTORY;
    jc = (long)null_bin * n_camera_bins + null_bin;
  }
  *joint_buttons = jb;
  *joint_camera = jc;
}
