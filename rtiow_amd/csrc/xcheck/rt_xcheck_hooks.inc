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
    const auto d_r1 = st.in(r1, 256), d_r2 = st.in(r2, 256), d_s = st.in(s, 64);
    const auto d_hb = st.out(out_hb, 1024), d_q = st.out(out_q, 1024);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.upload());
    hipLaunchKernelGGL(rt::filter_products_kernel, dim3(1), dim3(64), 0, ctx->own_stream,
                       st.ptr(d_r1), st.ptr(d_r2), st.ptr(d_s), (int)bf16x3, st.ptr(d_hb), st.ptr(d_q));
    RT_HIP(hipGetLastError());
    RT_HIP(st.finish());
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
    Stage st(ctx);
    const auto d_o = st.in(o, 64 * 3), d_d = st.in(d, 64 * 3);
    const auto d_tile = st.in(tile, 128);
    const auto d_D = st.out(out_D, 1024), d_R = st.out(out_R, 64 * (size_t)rt::kLiftTerms);
    int rc = st.commit();
    if (rc) return rc;
    RT_HIP(st.upload());
    hipLaunchKernelGGL(rt::lifted_products_kernel, dim3(1), dim3(64), 0, ctx->own_stream,
                       st.ptr(d_o), st.ptr(d_d), st.ptr(d_tile), st.ptr(d_D), st.ptr(d_R));
    RT_HIP(hipGetLastError());
    RT_HIP(st.finish());
    return RT_OK;
}


int rt_grid_cells_device(rt_context *ctx, const double *o, const double *d, int32_t n, const float grid[8], int32_t grid_dim, float scale,
                         int32_t *out_rect, int32_t *out_runs)
{
    if (!ctx || !o || !d || !grid || !out_rect || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (grid_dim < 1 || grid_dim > rt_scene::kMaxGridDim) return fail(RT_ERR_INVALID_ARGUMENT, "grid_dim must be 1..%d", rt_scene::kMaxGridDim);
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    int32_t bad = 0;
    Stage st(ctx);
    const auto d_o = st.in(o, (size_t)n * 3), d_d = st.in(d, (size_t)n * 3);
    const auto d_rect = st.out(out_rect, (size_t)n * 5), d_runs = st.out(out_runs, (size_t)n * 126);
    const auto d_bad = st.inout(&bad, 1);               // (goes up as 0)
    int rc = st.commit();
    if (rc) return rc;
    rt::GridArgs ga;
    for (int k = 0; k < 8; ++k) ga.g[k] = grid[k];
    RT_HIP(st.upload());
    hipLaunchKernelGGL(rt::grid_cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->own_stream,
                       st.ptr(d_o), st.ptr(d_d), (int)n, ga, (int)grid_dim, scale, st.ptr(d_rect), st.ptr(d_runs), st.ptr(d_bad));
    RT_HIP(hipGetLastError());
    RT_HIP(st.finish());
    if (bad) return fail(RT_ERR_HIP, "rt_grid_cells_device: grid_cells with and without GridSeg disagree on some ray");
    return RT_OK;
}
