// rt_xcheck_host.inc -- part of the CROSS-CHECK build only (-DRTIOW_CROSSCHECK_MODES: tools/librtiow_hip_xcheck.so, a test artefact).
// Host side of scan modes 2-4, the earlier matrix-pipe forms of the sphere-scan filter (DESIGN.md section 5.2); the product library carries
// modes 0, 1 and 5 and never includes this file.  Included inside namespace rt_host in rt_api.hip (after upload_table; filter_kprime and host_split_bf16x3 are rt_scene_core.hpp's): the B operands of modes 2-4.
// lifted_column and lifted_tile are declared in rt_xcheck_host_ctx.hpp: rt_filter_lifted_device (rt_xcheck_hooks.inc, rt_selftest.hip) calls them too.
// ---- MODE 4 (lifted form, rt_device.hpp): the per-sphere column C_0..C_10 and its 64 K-slots ----
// `s == nullptr` (padding) or `never` (a sphere on the always-exact list): a column no ray keeps.
// Every C_k is computed in f64 from the exact centre/radius and rounded once; C_10 = -K' is
// rounded UP (K' down), the conservative direction.
void lifted_column(const rt_sphere *s, bool never, float C[rt::kLiftTerms])
{
    for (int k = 0; k < rt::kLiftTerms; ++k) C[k] = 0.0f;
    C[0] = 1.0f;
    if (!s || never) { C[10] = rt::kLiftNever; return; }
    const float kp = rt_scene::filter_kprime(*s, (double)rt::kFilterKU_lifted);
    if (!(kp > -INFINITY)) { C[10] = rt::kLiftAlways; return; }       // outside the analysed range
    const double cx = s->center[0], cy = s->center[1], cz = s->center[2];
    C[1] = (float)cx; C[2] = (float)cy; C[3] = (float)cz;
    C[4] = (float)(cx * cx); C[5] = (float)(cy * cy); C[6] = (float)(cz * cz);
    C[7] = (float)(cx * cy); C[8] = (float)(cx * cz); C[9] = (float)(cy * cz);
    C[10] = -kp;
}
// B-side dwords of the slot layout documented at lifted_a_words()
static void lifted_b_words(const float C[rt::kLiftTerms], uint32_t w[32])
{
    for (int p = 0; p < 9; ++p) {
        uint32_t y[3]; rt_scene::host_split_bf16x3(C[1 + p], y);
        w[3 * p + 0] = y[0] | (y[1] << 16);
        w[3 * p + 1] = y[0] | (y[2] << 16);
        w[3 * p + 2] = y[1] | (y[0] << 16);
    }
    uint32_t k[3]; rt_scene::host_split_bf16x3(C[10], k);
    w[27] = rt::kBf16One | (rt::kBf16One << 16);      // C_0 = 1 against the three pieces of R_0
    w[28] = rt::kBf16One | (k[0] << 16);
    w[29] = k[1] | (k[2] << 16);
    w[30] = 0u; w[31] = 0u;
}
// one tile (16 columns) of the B table: [m][lane] uint4, lane l = column l&15, K-slots 32m + 8(l>>4)..+7
void lifted_tile(const float C[16][rt::kLiftTerms], uint4 out[128])
{
    for (int c = 0; c < 16; ++c) {
        uint32_t w[32]; lifted_b_words(C[c], w);
        for (int m = 0; m < 2; ++m)
            for (int quad = 0; quad < 4; ++quad) {
                const uint32_t *q = &w[4 * (4 * m + quad)];
                out[m * 64 + quad * 16 + c] = make_uint4(q[0], q[1], q[2], q[3]);
            }
    }
}


// the device tables of the scan mode the context runs (2: f32 B operand + K'; 3: three-piece bf16 B operand + K' at the larger KU; 4: lifted form)
static int xcheck_upload_tables(rt_context *ctx, const rt_sphere *spheres, int n, const rt_scene::Tables &T)
{
    int rc = RT_OK;
    const std::vector<float> &filt = T.filt;
    const rt_scene::Header &H = T.header;
    const int n_tiles = H.n_tiles;
    const size_t tcnt = (size_t)n_tiles + 2;
    if (ctx->scan_mode == 2 || ctx->scan_mode == 3) {
        std::vector<float> bmat(tcnt * 64, 0.0f), kpt(tcnt * 16, NAN);
        for (int t = 0; t < n_tiles + 2; ++t)
            for (int l = 0; l < 64; ++l) {
                const int i = 16 * t + (l & 15), k = l >> 4;
                float v = (k == 3) ? 1.0f : 0.0f;                  // padding columns: c = 0
                if (i < n && k < 3) v = filt[4 * i + k];
                bmat[(size_t)t * 64 + l] = v;
            }
        for (int i = 0; i < n; ++i) kpt[i] = filt[4 * i + 3];      // padding stays NaN: never kept
        for (int e = 0; e < H.n_always; ++e) kpt[H.always_idx[e]] = NAN;
        if (ctx->scan_mode == 2) {
            if (!rc) rc = upload_table(&ctx->x.d_bmat, bmat.data(), bmat.size());
            if (!rc) rc = upload_table(&ctx->x.d_kpt, kpt.data(), kpt.size());
        } else {
            // bf16x3 form: each S value as three bf16 pieces in the element order the A side pairs
            // with (rt_device.hpp, a_operand_bf16x3), and K' recomputed with that scheme's larger KU
            std::vector<uint4> bmat16(tcnt * 64, make_uint4(0u, 0u, 0u, 0u));
            std::vector<float> kpt16(tcnt * 16, NAN);
            for (size_t e = 0; e < bmat.size(); ++e) {
                uint32_t y[3]; rt_scene::host_split_bf16x3(bmat[e], y);
                bmat16[e] = make_uint4(y[0] | (y[1] << 16), y[0] | (y[2] << 16), y[1] | (y[0] << 16), y[2] | (y[1] << 16));
            }
            for (int i = 0; i < n; ++i) kpt16[i] = rt_scene::filter_kprime(spheres[i], (double)rt::kFilterKU_bf16x3);
            for (int e = 0; e < H.n_always; ++e) kpt16[H.always_idx[e]] = NAN;
            if (!rc) rc = upload_table(&ctx->x.d_bmat16, bmat16.data(), bmat16.size());
            if (!rc) rc = upload_table(&ctx->x.d_kpt16, kpt16.data(), kpt16.size());
        }
    }
    if (ctx->scan_mode == 4) {
        std::vector<uint4> bmatL(tcnt * 128);
        const int *always_end = H.always_idx + H.n_always;
        for (size_t t = 0; t < tcnt; ++t) {
            float C[16][rt::kLiftTerms];
            for (int c = 0; c < 16; ++c) {
                const long i = 16 * (long)t + c;
                lifted_column(i < n ? &spheres[i] : nullptr, i < n && std::find(H.always_idx, always_end, (int)i) != always_end, C[c]);
            }
            lifted_tile(C, &bmatL[t * 128]);
        }
        if (!rc) rc = upload_table(&ctx->x.d_bmatL, bmatL.data(), bmatL.size());
    }
    return rc;
}
