// rt_xcheck_hooks.inc -- part of the CROSS-CHECK build only (-DRTIOW_CROSSCHECK_MODES: tools/librtiow_hip_xcheck.so, a test artefact).
// Host side of scan modes 2-4, the earlier matrix-pipe forms of the sphere-scan filter (DESIGN.md section 5.2); the product library carries
// modes 0, 1 and 5 and never includes this file.  Included inside rt_selftest.hip's extern "C" block: the known-answer hooks the header declares under RTIOW_CROSSCHECK_MODES
// (those of modes 2-4, and rt_grid_cells_device: the shipped mode's grid footprint, kept out of the product ABI).
int rt_filter_products_device(rt_context *ctx, const float *r1, const float *r2, const float *s,
                               int32_t bf16x3, float *out_hb, float *out_q)
{
    if (!ctx || !r1 || !r2 || !s || !out_hb || !out_q) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_HIP(hipSetDevice(ctx->device));
    Stage st(ctx);
    const size_t b_r1 = st.add(256 * 4), b_r2 = st.add(256 * 4), b_s = st.add(64 * 4), b_hb = st.add(1024 * 4), b_q = st.add(1024 * 4);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.up(b_r1, r1, 256 * 4));
    RT_HIP(st.up(b_r2, r2, 256 * 4));
    RT_HIP(st.up(b_s, s, 64 * 4));
    hipLaunchKernelGGL(rt::filter_products_kernel, dim3(1), dim3(64), 0, ctx->own_stream,
                       st.at<const float>(b_r1), st.at<const float>(b_r2), st.at<const float>(b_s), (int)bf16x3, st.at<float>(b_hb), st.at<float>(b_q));
    RT_HIP(hipGetLastError());
    RT_HIP(st.down(out_hb, b_hb, 1024 * 4));
    RT_HIP(st.down(out_q, b_q, 1024 * 4));
    RT_HIP(st.sync());
    return RT_OK;
}

int rt_filter_lifted_device(rt_context *ctx, const double *o, const double *d, const rt_sphere *spheres16,
                            float *out_D, float *out_R, float *out_C)
{
    if (!ctx || !o || !d || !spheres16 || !out_D || !out_R || !out_C) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_HIP(hipSetDevice(ctx->device));
    float C[16][rt::kLiftTerms];
    for (int c = 0; c < 16; ++c) lifted_column(&spheres16[c], false, C[c]);
    memcpy(out_C, C, sizeof(C));
    uint4 tile[128];
    lifted_tile(C, tile);
    const size_t R_b = 64 * rt::kLiftTerms * 4;
    Stage st(ctx);
    const size_t b_o = st.add(1536), b_d = st.add(1536), b_tile = st.add(sizeof(tile)), b_D = st.add(1024 * 4), b_R = st.add(R_b);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.up(b_o, o, 1536));
    RT_HIP(st.up(b_d, d, 1536));
    RT_HIP(st.up(b_tile, tile, sizeof(tile)));
    hipLaunchKernelGGL(rt::lifted_products_kernel, dim3(1), dim3(64), 0, ctx->own_stream,
                       st.at<const double>(b_o), st.at<const double>(b_d), st.at<const uint4>(b_tile), st.at<float>(b_D), st.at<float>(b_R));
    RT_HIP(hipGetLastError());
    RT_HIP(st.down(out_D, b_D, 1024 * 4));
    RT_HIP(st.down(out_R, b_R, R_b));
    RT_HIP(st.sync());
    return RT_OK;
}


int rt_grid_cells_device(rt_context *ctx, const double *o, const double *d, int32_t n, const float grid[8], int32_t grid_dim, float scale,
                         int32_t *out_rect, int32_t *out_runs)
{
    if (!ctx || !o || !d || !grid || !out_rect || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (grid_dim < 1 || grid_dim > rt_scene::kMaxGridDim) return fail(RT_ERR_INVALID_ARGUMENT, "grid_dim must be 1..%d", rt_scene::kMaxGridDim);
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const size_t ob = (size_t)n * 3 * sizeof(double), rb = (size_t)n * 5 * sizeof(int32_t), wb = out_runs ? (size_t)n * 126 * sizeof(int32_t) : 0;
    Stage st(ctx);
    const size_t b_o = st.add(ob), b_d = st.add(ob), b_rect = st.add(rb), b_runs = st.add(wb), b_bad = st.add(sizeof(int32_t));
    int rc = st.commit();
    if (rc) return rc;
    rt::GridArgs ga;
    for (int k = 0; k < 8; ++k) ga.g[k] = grid[k];
    RT_HIP(st.up(b_o, o, ob));
    RT_HIP(st.up(b_d, d, ob));
    RT_HIP(hipMemsetAsync(st.at(b_bad), 0, sizeof(int32_t), ctx->own_stream));
    hipLaunchKernelGGL(rt::grid_cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->own_stream,
                       st.at<const double>(b_o), st.at<const double>(b_d), (int)n, ga, (int)grid_dim, scale, st.at<int32_t>(b_rect),
                       out_runs ? st.at<int32_t>(b_runs) : nullptr, st.at<int32_t>(b_bad));
    RT_HIP(hipGetLastError());
    int32_t bad = 0;
    RT_HIP(st.down(out_rect, b_rect, rb));
    if (out_runs) RT_HIP(st.down(out_runs, b_runs, wb));
    RT_HIP(st.down(&bad, b_bad, sizeof(int32_t)));
    RT_HIP(st.sync());
    if (bad) return fail(RT_ERR_HIP, "rt_grid_cells_device: grid_cells with and without GridSeg disagree on some ray");
    return RT_OK;
}
