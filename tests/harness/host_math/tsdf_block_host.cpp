// TEST INFRASTRUCTURE (tests/test_tsdf_block_rule_on_host.py): the PRODUCT's csrc/tsdf_block_rule.h and csrc/tsdf_rule.h
// -- copied next to this file at test time, never edited -- compiled for the host; their "common.h" is the stand-in
// beside this file.  A program of its own: it reads one marking job from the file named by argv[1] and writes the marks
// and the block of every marched point to the file named by argv[2].
//
//   in   int32 W, H, nx, ny, nz, has_weight; float view[12], tanfovx, tanfovy, z_min, lo[3], voxel, trunc;
//        float depth[H W]; float weight[H W] (if has_weight)
//   out  int32 S, refused, gx, gy, gz; uint8 marks[gz gy gx]; int32 n_points; int32 points[n_points][5] = (px, py,
//        bi, bj, bk) in marching order
#include "tsdf_block_rule.h"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t head[6];
  float par[20];
  if (fread(head, 4, 6, in) != 6 || fread(par, 4, 20, in) != 20) return 4;
  const int32_t W = head[0], H = head[1];
  const size_t n = (size_t)W * (size_t)H;
  std::vector<float> depth(n), weight(n);
  if (fread(depth.data(), 4, n, in) != n) return 4;
  if (head[5] && fread(weight.data(), 4, n, in) != n) return 4;
  fclose(in);
  const float* view = par;
  const float tanfovx = par[12], tanfovy = par[13], z_min = par[14], voxel = par[18], trunc = par[19];
  const float lo[3] = {par[15], par[16], par[17]};
  const int32_t grid[3] = {hgs::tsdf_block_grid(head[2]), hgs::tsdf_block_grid(head[3]), hgs::tsdf_block_grid(head[4])};
  const int32_t S = hgs::tsdf_block_steps(trunc, voxel);
  std::vector<uint8_t> marks((size_t)grid[0] * grid[1] * grid[2], 0);
  std::vector<int32_t> points;
  int32_t refused = 0;
  if (S <= hgs::kTsdfMaxSteps) {
    for (int32_t py = 0; py < H; ++py)
      for (int32_t px = 0; px < W; ++px) {
        const size_t pix = (size_t)py * W + px;
        const bool marched = hgs::tsdf_block_march(
            px, py, depth[pix], head[5] ? weight[pix] : 1.0f, view, tanfovx, tanfovy, W, H, z_min, lo, voxel, trunc, S, grid,
            [&](int32_t bi, int32_t bj, int32_t bk) {
              marks[((size_t)bk * grid[1] + bj) * grid[0] + bi] = 1;
              const int32_t row[5] = {px, py, bi, bj, bk};
              points.insert(points.end(), row, row + 5);
            });
        if (!marched) refused = 1;
      }
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 5;
  const int32_t first[5] = {S, refused, grid[0], grid[1], grid[2]};
  const int32_t count = (int32_t)(points.size() / 5);
  fwrite(first, 4, 5, out);
  fwrite(marks.data(), 1, marks.size(), out);
  fwrite(&count, 4, 1, out);
  fwrite(points.data(), 4, points.size(), out);
  fclose(out);
  return 0;
}
