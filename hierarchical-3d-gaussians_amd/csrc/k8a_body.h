// The body of K8a's two kernels (preprocess.hip: preprocess_bwd_kernel<ACC, LOD>, preprocess_bwd_staged_kernel<ACC>), included
// into each with ACC, LOD and STG in scope as constants.  Text, not a function: as a forced-inline function with the same
// parameters the compiler needs 176 - 180 registers for it instead of 156 - 158, and the kernels fall to two waves per SIMD.
  const int idx = blockIdx.x * kPreBlock + threadIdx.x;
  const bool in_range = idx < a.P;
  static_assert(kInstStride == 10, "instance record = the ten sums, 40 bytes");
  __shared__ __attribute__((aligned(16))) float2 stage[kPreBlock / 64][kK8StageRec * 5];
  __shared__ __attribute__((aligned(16))) unsigned char staged_in[STG ? (kPreBlock / 64) * kK8InWave : 16];
  const int wave = threadIdx.x >> 6;
  const unsigned char* in = staged_in + (STG ? wave * kK8InWave : 0);
  CamLds cam;
  if constexpr (STG) {
    load_camera(a, cam);
    k8_stage_inputs(a, g, idx, mode, staged_in + wave * kK8InWave);
  }
  const uint32_t n = in_range ? g.tiles_touched[idx] : 0u;   // (out-of-range lanes stay for the wave-wide staging below)
  uint32_t off = 0u;
  if constexpr (STG) { if (in_range) off = g.offsets[idx]; }
  else { if (n) off = g.offsets[idx]; }

  double s[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) s[i] = 0.0;
  k8_sum_runs<STG>(inst, off, n, mode, stage[wave], s);
  if constexpr (STG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (a wave that staged no records: the inputs have landed)
  if constexpr (!LOD) {
    if (!in_range) return;
  }

  float d_mean[3] = {0.f, 0.f, 0.f};
  float d_m2[3] = {0.f, 0.f, 0.f};
  float d_op = 0.f;
  float d_scale[3] = {0.f, 0.f, 0.f};
  float d_rot[4] = {0.f, 0.f, 0.f, 0.f};
  float d_c3[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float gr[3] = {0.f, 0.f, 0.f};
  float d_col[3] = {0.f, 0.f, 0.f};
  if (n != 0) {                              // (culled: all-zero gradients; K8b zero-fills dL/dSH)
    float p[3];
    k8_chain<LOD, STG>(a, g, idx, s, p, d_mean, d_m2, d_op, d_scale, d_rot, d_c3, gr, in, &cam);
    // colour: precomputed colours get their gradient here; SH colours hand the clamp-masked dL/drgb to K8b
    if (a.colors_precomp) {
      d_col[0] = gr[0]; d_col[1] = gr[1]; d_col[2] = gr[2];
    } else {
      drgb[idx * 3 + 0] = gr[0];
      drgb[idx * 3 + 1] = gr[1];
      drgb[idx * 3 + 2] = gr[2];
    }
  }

  if constexpr (LOD) {
    if (a.lod_scatter) {
      // scales, rotations, opacity: scattered here; the mean's gradient goes on to K8b (which adds the view-direction
      // term and scatters it together with the SH gradients)
      __shared__ float lds_v[8 * kPreBlock];
      __shared__ int lds_par[kPreBlock];
      __shared__ unsigned char lds_vis[kPreBlock];
      const int t = threadIdx.x;
      const int block_first = blockIdx.x * kPreBlock;
      const int count = min(kPreBlock, a.P - block_first);
      LodRow l;
      l.r = l.p = 0; l.w = 1.0f; l.u = 0.0f;
      if (in_range) l = lod_row<true>(a, idx);
      const bool self = l.p == l.r;
      const bool vis = in_range && n != 0;
      const float wn = self ? 1.0f : l.w, u = (self || !vis) ? 0.0f : l.u;
      float sgn = 1.0f;
      if (vis && !self && u != 0.0f) {          // (weight 1: nothing goes to the parent, its quaternion is not needed)
        const float4 qa = reinterpret_cast<const float4*>(a.rotations)[l.r];
        const float4 qb = reinterpret_cast<const float4*>(a.rotations)[l.p];
        sgn = (qa.x * qb.x + qa.y * qb.y + qa.z * qb.z + qa.w * qb.w) < 0.0f ? -1.0f : 1.0f;
      }
      if (in_range) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          dmean_rows[idx * 3 + j] = d_mean[j];
          out.dL_dmeans2D[idx * 3 + j] = d_m2[j];
        }
      }
      if (vis) {      // node row (culled rows have zero gradients: the caller's zero fill stands)
        out.dL_dopacity[l.r] = wn * d_op;
#pragma unroll
        for (int j = 0; j < 3; ++j) out.dL_dscales[l.r * 3 + j] = wn * d_scale[j];
        reinterpret_cast<float4*>(out.dL_drotations)[l.r] = make_float4(wn * d_rot[0], wn * d_rot[1], wn * d_rot[2], wn * d_rot[3]);
      }
      lds_par[t] = in_range ? (int)l.p : -1;
      lds_vis[t] = (vis && !self) ? 1 : 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) lds_v[j * kPreBlock + t] = u * d_scale[j];
#pragma unroll
      for (int j = 0; j < 4; ++j) lds_v[(3 + j) * kPreBlock + t] = (u * sgn) * d_rot[j];
      lds_v[7 * kPreBlock + t] = u * d_op;
      __syncthreads();
      if (t < count) {
        const LodRun run = lod_run(a, lds_par, t, count, block_first, *lod_flag != 0u);
        if (run.leader) {
          float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          bool any = false;
          for (int j = t; j < run.end; ++j) {
            if (!lds_vis[j]) continue;
            any = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc8[k] += lds_v[k * kPreBlock + j];
          }
          if (any) {
            const size_t pp = (size_t)lds_par[t];
#pragma unroll
            for (int k = 0; k < 3; ++k) lod_add(out.dL_dscales + pp * 3 + k, acc8[k], run.atomic);
#pragma unroll
            for (int k = 0; k < 4; ++k) lod_add(out.dL_drotations + pp * 4 + k, acc8[3 + k], run.atomic);
            lod_add(out.dL_dopacity + pp, acc8[7], run.atomic);
          }
        }
      }
      return;
    }
    if (!in_range) return;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) out.dL_dmeans3D[idx * 3 + j] = d_mean[j] + (ACC ? out.dL_dmeans3D[idx * 3 + j] : 0.f);
  k8_store_row<ACC>(out, idx, d_m2, d_op, d_scale, d_rot, d_c3, d_col);
