// Host-side check of the augmentation's per-pixel code (csrc/vpt_augment_pixel.h, the function vpt_augment_frames_kernel runs): a stand-alone program,
// built by tests/test_augment_host_cpu.py as plain C++ with contraction off and the address and undefined-behaviour sanitizers (host code only).
//
// Every frame lives in a heap block of exactly H * W * 3 bytes, so a tap outside the frame is an AddressSanitizer report.  Every pixel of every frame
// size is run under tables that hold NaN, +-Inf, +-1e30 and denormals in each of the 16 positions, and under random in-range tables.  The outputs of the
// tables whose entries are all finite are written to the file named on the command line, with their inputs, for the test to compare with
// tests/augment_ref.py:
//     int32 count;  count x { int32 H, W;  float table[16];  uint8 src[H*W*3];  uint8 out[H*W*3] }
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../video-pre-training_amd/csrc/vpt_augment_pixel.h"

static uint32_t g_state = 0x2545F491u;
static uint32_t next_u32() { g_state = g_state * 1664525u + 1013904223u; return g_state; }
static float next_unit() { return (float)(next_u32() >> 8) * (1.0f / 16777216.0f); }

static const float kIdentity[16] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0};

static bool all_finite(const float* t) {
  for (int i = 0; i < 16; ++i) if (!std::isfinite(t[i])) return false;
  return true;
}

static void run_frame(const uint8_t* src, int H, int W, const float* table, uint8_t* out) {
  int lum = 0;
  for (int p = 0; p < H * W; ++p) lum += VPT_AUG_LUMA_R * src[3 * p] + VPT_AUG_LUMA_G * src[3 * p + 1] + VPT_AUG_LUMA_B * src[3 * p + 2];
  const float inv = (float)(1.0 / (256.0 * (double)H * (double)W));
  const float mu = vpt_augment_mean(lum, inv);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) vpt_augment_pixel(src, H, W, table, mu, x, y, out + (y * W + x) * 3);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <output file>\n", argv[0]); return 2; }
  FILE* fo = fopen(argv[1], "wb");
  if (!fo) { perror(argv[1]); return 2; }
  const float inf = std::numeric_limits<float>::infinity();
  const float special[] = {std::numeric_limits<float>::quiet_NaN(), inf, -inf, 1e30f, -1e30f, std::numeric_limits<float>::denorm_min(), -1e-40f};
  const int sizes[4][2] = {{5, 7}, {16, 16}, {33, 20}, {128, 128}};
  int32_t count = 0, ran = 0;
  fwrite(&count, 4, 1, fo);                                     // patched at the end
  for (int s = 0; s < 4; ++s) {
    const int H = sizes[s][0], W = sizes[s][1], n = H * W * 3;
    uint8_t* src = (uint8_t*)malloc(n);                         // exactly the frame: one byte further is a sanitizer report
    uint8_t* out = (uint8_t*)malloc(n);
    for (int i = 0; i < n; ++i) src[i] = (uint8_t)(next_u32() >> 24);
    std::vector<std::vector<float>> tables;
    for (int pos = 0; pos < 16; ++pos)
      for (float v : special) {
        std::vector<float> t(kIdentity, kIdentity + 16);
        t[pos] = v;
        tables.push_back(t);
      }
    for (int k = 0; k < 2; ++k) {                               // everything special at once
      std::vector<float> t(16);
      for (int i = 0; i < 16; ++i) t[i] = special[(i + 3 * k) % 7];
      tables.push_back(t);
    }
    for (int k = 0; k < 8; ++k) {                               // random in-range tables: colour and warp near the identity, a few pixels of translation
      std::vector<float> t(kIdentity, kIdentity + 16);
      for (int i = 0; i < 9; ++i) t[i] += (next_unit() - 0.5f) * 0.6f;
      t[9] = (next_unit() - 0.5f) * 0.5f;
      for (int i = 10; i < 16; ++i) t[i] += (next_unit() - 0.5f) * ((i == 12 || i == 15) ? 12.0f : 0.3f);
      tables.push_back(t);
    }
    for (const auto& t : tables) {
      memset(out, 0xAA, n);
      run_frame(src, H, W, t.data(), out);
      ++ran;
      if (!all_finite(t.data())) continue;
      const int32_t hw[2] = {H, W};
      fwrite(hw, 4, 2, fo);
      fwrite(t.data(), 4, 16, fo);
      fwrite(src, 1, n, fo);
      fwrite(out, 1, n, fo);
      ++count;
    }
    free(src);
    free(out);
  }
  fseek(fo, 0, SEEK_SET);
  fwrite(&count, 4, 1, fo);
  if (fclose(fo) != 0) return 2;
  printf("augment_host_check: %d tables run, %d finite ones written\n", ran, count);
  return 0;
}
