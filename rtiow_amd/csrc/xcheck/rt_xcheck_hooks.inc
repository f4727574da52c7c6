// rt_xcheck_hooks.inc -- part of the CROSS-CHECK build only (-DRTIOW_CROSSCHECK_MODES: tools/librtiow_hip_xcheck.so, a test artefact).
// Host side of scan modes 2-4, the earlier matrix-pipe forms of the sphere-scan filter (DESIGN.md section 5.2); the product library carries
// modes 0, 1 and 5 and never includes this file.  Included inside rt_api.hip's extern "C" block: the known-answer hooks the header declares under RTIOW_CROSSCHECK_MODES
// (those of modes 2-4, and rt_grid_cells_device: the shipped mode's grid footprint, kept out of the product ABI).
int rt_filter_products_device(rt_context *ctx, const float *r1, const float *r2, const float *s,
                               int32_t bf16x3, float *out_hb, float *out_q)
{
    if (!ctx || !r1 || !r2 || !s || !out_hb || !out_q) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t in_f = 64 * 4 * 2 + 16 * 4, out_f = 64 * 16 * 2;
    int rc = ensure(&ctx->d_stage_fix, &ctx->stage_fix_bytes, (in_f + out_f) * sizeof(float));
    if (rc) return rc;
    float *d = (float *)ctx->d_stage_fix;
    float *d_r1 = d, *d_r2 = d + 256, *d_s = d + 512, *d_hb = d + 576, *d_q = d + 576 + 1024;
    RT_HIP(hipMemcpyAsync(d_r1, r1, 256 * 4, hipMemcpyHostToDevice, ctx->own_stream));
    RT_HIP(hipMemcpyAsync(d_r2, r2, 256 * 4, hipMemcpyHostToDevice, ctx->own_stream));
    RT_HIP(hipMemcpyAsync(d_s, s, 64 * 4, hipMemcpyHostToDevice, ctx->own_stream));
    hipLaunchKernelGGL(rt::filter_products_kernel, dim3(1), dim3(64), 0, ctx->own_stream,
                       (const float *)d_r1, (const float *)d_r2, (const float *)d_s, (int)bf16x3, d_hb, d_q);
    RT_HIP(hipGetLastError());
    RT_HIP(hipMemcpyAsync(out_hb, d_hb, 1024 * 4, hipMemcpyDeviceToHost, ctx->own_stream));
    RT_HIP(hipMemcpyAsync(out_q, d_q, 1024 * 4, hipMemcpyDeviceToHost, ctx->own_stream));
    RT_HIP(hipStreamSynchronize(ctx->own_stream));
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
    const size_t in_b = 64 * 3 * 8 * 2 + sizeof(tile), out_b = (64 * 16 + 64 * rt::kLiftTerms) * 4;
    int rc = ensure(&ctx->d_stage_fix, &ctx->stage_fix_bytes, in_b + out_b);
    if (rc) return rc;
    char *base = (char *)ctx->d_stage_fix;
    double *d_o = (double *)base, *d_d = d_o + 192;
    uint4 *d_tile = (uint4 *)(base + 3072);
    float *d_D = (float *)(base + 3072 + sizeof(tile)), *d_R = d_D + 1024;
    RT_HIP(hipMemcpyAsync(d_o, o, 1536, hipMemcpyHostToDevice, ctx->own_stream));
    RT_HIP(hipMemcpyAsync(d_d, d, 1536, hipMemcpyHostToDevice, ctx->own_stream));
    RT_HIP(hipMemcpyAsync(d_tile, tile, sizeof(tile), hipMemcpyHostToDevice, ctx->own_stream));
    hipLaunchKernelGGL(rt::lifted_products_kernel, dim3(1), dim3(64), 0, ctx->own_stream,
                       (const double *)d_o, (const double *)d_d, (const uint4 *)d_tile, d_D, d_R);
    RT_HIP(hipGetLastError());
    RT_HIP(hipMemcpyAsync(out_D, d_D, 1024 * 4, hipMemcpyDeviceToHost, ctx->own_stream));
    RT_HIP(hipMemcpyAsync(out_R, d_R, 64 * rt::kLiftTerms * 4, hipMemcpyDeviceToHost, ctx->own_stream));
    RT_HIP(hipStreamSynchronize(ctx->own_stream));
    return RT_OK;
}


int rt_grid_cells_device(rt_context *ctx, const double *o, const double *d, int32_t n, const float grid[8], int32_t grid_dim, float scale,
                         int32_t *out_rect, int32_t *out_runs)
{
    if (!ctx || !o || !d || !grid || !out_rect || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (grid_dim < 1 || grid_dim > kMaxGridDim) return fail(RT_ERR_INVALID_ARGUMENT, "grid_dim must be 1..%d", kMaxGridDim);
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const size_t ob = (size_t)n * 3 * sizeof(double), rb = (size_t)n * 5 * sizeof(int32_t), wb = out_runs ? (size_t)n * 126 * sizeof(int32_t) : 0;
    int rc = ensure(&ctx->d_stage_fix, &ctx->stage_fix_bytes, 2 * ob + rb + wb + 16);
    if (rc) return rc;
    char *base = (char *)ctx->d_stage_fix;
    double *d_o = (double *)base, *d_d = (double *)(base + ob);
    int32_t *d_rect = (int32_t *)(base + 2 * ob), *d_runs = out_runs ? (int32_t *)(base + 2 * ob + rb) : nullptr;
    int32_t *d_bad = (int32_t *)(base + 2 * ob + rb + wb);
    rt::GridArgs ga;
    for (int k = 0; k < 8; ++k) ga.g[k] = grid[k];
    RT_HIP(hipMemcpyAsync(d_o, o, ob, hipMemcpyHostToDevice, ctx->own_stream));
    RT_HIP(hipMemcpyAsync(d_d, d, ob, hipMemcpyHostToDevice, ctx->own_stream));
    RT_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), ctx->own_stream));
    hipLaunchKernelGGL(rt::grid_cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->own_stream,
                       (const double *)d_o, (const double *)d_d, (int)n, ga, (int)grid_dim, scale, d_rect, d_runs, d_bad);
    RT_HIP(hipGetLastError());
    int32_t bad = 0;
    RT_HIP(hipMemcpyAsync(out_rect, d_rect, rb, hipMemcpyDeviceToHost, ctx->own_stream));
    if (out_runs) RT_HIP(hipMemcpyAsync(out_runs, d_runs, wb, hipMemcpyDeviceToHost, ctx->own_stream));
    RT_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->own_stream));
    RT_HIP(hipStreamSynchronize(ctx->own_stream));
    if (bad) return fail(RT_ERR_HIP, "rt_grid_cells_device: grid_cells with and without GridSeg disagree on some ray");
    return RT_OK;
}
