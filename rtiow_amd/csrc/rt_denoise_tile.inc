// rt_denoise_tile.inc -- the body of the tile form of both level kernels, included textually into each __global__ function (a template
// body called from them keeps neither kernel's instruction order: DESIGN.md section 15).  In scope: the frame F, the tiling T, and the
// unit's dn_tile_pixel(F, i, j, W, H, centre, staged), which filters one pixel and stores it.
    using Rec = decltype(F)::Rec;
    __shared__ double s_rec[kDnPlanes<Rec>][kDnCells];
    const long long s = F.L.step;
    const long long W = (long long)F.width, H = (long long)F.height;
    const int lx = (int)threadIdx.x & (kDnTile - 1), ly = (int)threadIdx.x >> 4;
    const uint32_t gx = T.nri * T.tiles_x;
    for (uint32_t t = blockIdx.x; t < T.n_tiles; t += gridDim.x) {
        const uint32_t by = t / gx, bx = t - by * gx;
        const uint32_t ri = bx / T.tiles_x, tx = bx - ri * T.tiles_x;
        const uint32_t rj = by / T.tiles_y, ty = by - rj * T.tiles_y;
        // sub-lattice coordinates (u, v) -> pixel (ri + s u, rj + s v); the tile's first cell is (16 tx - 2, 16 ty - 2)
        const long long u0 = (long long)tx * kDnTile - 2, v0 = (long long)ty * kDnTile - 2;
        for (int cell = (int)threadIdx.x; cell < kDnCells; cell += kDnBlock) {
            const int cy = cell / kDnSide, cx = cell - cy * kDnSide;
            const long long ii = (long long)ri + s * (u0 + cx), jj = (long long)rj + s * (v0 + cy);
            if (ii < 0 || ii >= W || jj < 0 || jj >= H) continue;           // never read: the pixel function skips taps outside the frame
            Rec r;
            dn_load_tap(F, (unsigned long long)(jj * W + ii), &r);
            dn_stage(s_rec, cell, r);
        }
        __syncthreads();
        const long long i = (long long)ri + s * (u0 + 2 + lx), j = (long long)rj + s * (v0 + 2 + ly);
        if (i < W && j < H) {
            auto staged = [&](int dx, int dy, Rec *q) { dn_staged(s_rec, (ly + 2 + dy) * kDnSide + (lx + 2 + dx), q); };
            Rec centre;
            staged(0, 0, &centre);
            dn_tile_pixel(F, i, j, W, H, centre, staged);
        }
        __syncthreads();                                                    // the next tile overwrites the records
    }
