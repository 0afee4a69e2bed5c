// pixie_amd/csrc/frame_export_body.h -- the per-particle body of the rasteriser hand-off (see frame_export_kernel in mpm.hip).
// Included INSIDE the two kernels that run it -- frame_export_kernel (one scene, parameters as kernel arguments) and
// frame_export_batch_kernel (several scenes, parameters from the per-scene descriptor and export record) -- after they have
// defined, in scope:
//   MpmPtrs S;  const float* init_cov;  FrameXform X;  int n_out;  float* pos_out, cov_out (this frame's outputs; cov_out may be
//   NULL);  int i: the particle row (storage order) this thread exports.
// (Textual inclusion, as mpm_block_body.h: the batched kernel must produce the solo kernel's bits, and the same statements moved
// into a function or read through references may contract other multiply-adds.)
// No include guard: included once per kernel.
    if (i >= S.n) return;
    const int s = S.perm[i];
    if (s >= n_out) return;
    float q[3];
    for (int d = 0; d < 3; ++d) q[d] = X.mean[d] + (S.x[(size_t)d * S.n + i] - X.shift[d]) * X.inv_scale;
    for (int d = 0; d < 3; ++d) pos_out[(size_t)s * 3 + d] = q[0] * X.M[d] + q[1] * X.M[3 + d] + q[2] * X.M[6 + d];
    if (!cov_out) return;
    Mat3 F, C0, M;
    for (int c = 0; c < 9; ++c) { F.m[c] = S.Ft[(size_t)c * S.n + i]; M.m[c] = X.M[c]; }
    const float* c6 = init_cov + (size_t)s * 6;
    C0.m[0] = c6[0]; C0.m[1] = c6[1]; C0.m[2] = c6[2];
    C0.m[3] = c6[1]; C0.m[4] = c6[3]; C0.m[5] = c6[4];
    C0.m[6] = c6[2]; C0.m[7] = c6[4]; C0.m[8] = c6[5];
    Mat3 T = mat_mul_bt(mat_mul(F, C0), F);                 // F C0 F^T
    for (int c = 0; c < 9; ++c) T.m[c] *= X.inv_scale2;
    // M^T T M
    Mat3 Mt;
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) Mt.m[3 * a + b] = M.m[3 * b + a];
    const Mat3 Rr = mat_mul(mat_mul(Mt, T), M);
    float* o = cov_out + (size_t)s * 6;
    o[0] = Rr.m[0]; o[1] = Rr.m[1]; o[2] = Rr.m[2]; o[3] = Rr.m[4]; o[4] = Rr.m[5]; o[5] = Rr.m[8];
