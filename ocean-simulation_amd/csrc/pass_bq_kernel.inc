// Pass BQ's kernel (fftq.hip, which documents it and includes this text twice): OCEAN_BQ_DT false = k_pass_bq,
// true = turb_deferred::k_pass_bq, the same item without the TURB store.
template <int N, bool BAND = false, int WT = 0, bool DC = false, bool PRUNE = false>
__global__ __launch_bounds__((WT ? WT : b3_w(N)) * N / kElems) void k_pass_bq(DevView v, int items, BqExtents<PRUNE> pe) {
    constexpr bool DT = OCEAN_BQ_DT;
    static_assert(!(PRUNE && BAND), "column-band contexts run the dense schedule");
    static_assert(!(DT && BAND), "a column-band frame writes TURB");
    using CT = ColTile<N, WT ? WT : b3_w(N)>;
    using E = typename CT::E;
    using TW = typename CT::TW;
    constexpr int W = CT::W;
    constexpr int T = CT::T;
    constexpr int RL = CT::RL;
    constexpr int TILE = W * N;
    constexpr bool kKeepLds = (E::LDS_ELEMS + TW::kLdsEntries + kElems * T + N) * 8 <= 160 * 1024;
    __shared__ float2 lds[E::LDS_ELEMS];
    __shared__ float2 twl[TW::kLdsEntries];
    __shared__ float2 keep_lds[kKeepLds ? kElems * T : 1];
    __shared__ float dks[kMaxCascades];
    __shared__ float2 d0s[N];  // the item's d0, staged through LDS instead of 16 registers per lane
    constexpr int DPL = (N + T - 1) / T;  // d0 entries each lane stages
    TW::load(twl, v.tw, threadIdx.x, T);
    const float2* tws = TW::table(twl, v.tw);
    if ((int)threadIdx.x < v.C) dks[threadIdx.x] = wave_band(v.casc + threadIdx.x * 5).dk;
    const int lb = CT::lane_b(), lj = CT::lane_j();
    const int toff = lj * W + lb;
    const int voff16 = (lj * N + lb) * 16;

    float2 keep_reg[kKeepLds ? 1 : kElems];
    auto kput = [&](int i, float2 x) {
        if constexpr (kKeepLds) keep_lds[i * T + threadIdx.x] = x;
        else keep_reg[i] = x;
    };
    auto kget = [&](int i) -> float2 {
        if constexpr (kKeepLds) return keep_lds[i * T + threadIdx.x];
        else return keep_reg[i];
    };
    // item -> full tile index u * tiles + tile over the column band's tiles
    const int bt0 = v.x0 / W, bnt = v.nx / W;
    // Without DC (chunked frames, as cfg4's) the 32 workgroups of one XCD (blocks b, b + 8, ...) take 32
    // consecutive tiles at each step of the item loop, so each XCD streams whole 256-column runs of the
    // texture rows: cfg4 51.2 -> 52.0 k tile-frames/s (G = 64 the same, 128 slower); at cfg3 (DC) it does
    // not help (docs/MEASUREMENTS.md section 8).  Needs items % (8 G) == 0, else the identity order.
    constexpr int G = DC ? 1 : 32;
    const bool grp = G > 1 && items % (8 * G) == 0;
    auto full = [&](int item) {
        if (grp) item = (item & ~(8 * G - 1)) + G * (item & 7) + ((item >> 3) & (G - 1));
        return BAND ? (item / bnt) * CT::tiles + bt0 + item % bnt : item;
    };
    auto win16 = [&](const float4* base, int ft) {
        const int u = ft / CT::tiles, x0 = (ft % CT::tiles) * W;
        return make_win(base + (size_t)u * N * N + x0, (unsigned)((N * N - x0) * 16));
    };
    auto extent_of = [&](int u) {
        if constexpr (PRUNE) return (int)((const cint_t*)pe.ext)[u];
        else return N / 2;
    };
    constexpr int kDeadOff = 0x40000000;  // a lane offset past every window (TILE * 8 bytes), scalar offsets included
    // row y of a unit of extent m is live iff |y - N/2| <= m: none of a flat unit's (m = -1, a uniform test)
    auto is_live = [&](int y, int m) { return m >= 0 && (unsigned)(y - (N / 2 - m)) <= (unsigned)(2 * m); };
    auto load = [&](int item, int p, float2 (&d)[kElems]) {
        const Win w = make_win(v.tplane + (size_t)p * v.inter_stride + (size_t)full(item) * TILE, TILE * 8);
        if constexpr (PRUNE) {
            const int m = extent_of(full(item) / CT::tiles);
#pragma unroll
            for (int i = 0; i < kElems; ++i) {
                const int vo = is_live(lj + CT::in_dy(i), m) ? toff * 8 : kDeadOff;
                d[i] = DC ? bload2<2>(w, vo, CT::in_dy(i) * W * 8) : bload2(w, vo, CT::in_dy(i) * W * 8);
            }
            return;
        }
        // DC: the intermediate's loads are nontemporal too (it is dead once read), which leaves DISP the
        // cache room; together +1.1-2.1 % at cfg3.  Without DC (chunked frames) they stay default-policy: at cfg4
        // nontemporal loads measured -1.1 to +1.1 % on two boxes (docs/MEASUREMENTS.md section 8)
#pragma unroll
        for (int i = 0; i < kElems; ++i)
            d[i] = DC ? bload2<2>(w, toff * 8, CT::in_dy(i) * W * 8) : bload2(w, toff * 8, CT::in_dy(i) * W * 8);
    };

    float2 cur[kElems], nxt[kElems], nx2[kElems], dd[DPL], srow = make_float2(0.0f, 0.0f);
    float kreg[kElems];
    int item = blockIdx.x;
    if (item < items) {
        load(item, 1, cur);  // R[Q2]
        load(item, 0, nxt);  // R[Q1]
    }
    __syncthreads();
    for (; item < items; item += gridDim.x) {
        const int ft = full(item);
        const int u = ft / CT::tiles;
        const int x0 = (ft % CT::tiles) * W;
        const float dk = dks[(u + v.c0) % v.C];
        float* foam = v.foam + (size_t)ft * TILE + toff;
        float fb[kElems];
        const bool more = item + (int)gridDim.x < items;
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            if (st == 0) {  // side values for step 1: the unit's d0 and, on row-0 lanes, srow
                const float2* side = q_side(v, u);
                const int m = extent_of(u);
#pragma unroll
                for (int k = 0; k < DPL; ++k) {
                    const int y = k * T + (int)threadIdx.x;
                    if (PRUNE) dd[k] = make_float2(0.0f, 0.0f);
                    if (y < N && (!PRUNE || is_live(y, m))) dd[k] = side[y];
                }
                if (PRUNE) srow = make_float2(0.0f, 0.0f);
                if (lj == 0 && m == N / 2) srow = side[N + x0 + lb];
                load(item, 2, nx2);  // R[Q3]
            } else if (st == 1) {
                // R[Q4] = i kz R[Q1] + d0 (row 0: srow) into the free ring slot
#pragma unroll
                for (int r = 0; r < kElems; ++r) {
                    const int y = lj + CT::in_dy(r);
                    const float kz = (float)(y - N / 2) * dk;
                    const float2 c = cur[r], d = d0s[y];
                    nx2[r] = make_float2(d.x - kz * c.y, d.y + kz * c.x);
                }
                if (lj == 0) nx2[0] = srow;
            } else {
                if (st == 2) {  // foam state for step 3, ahead of this step's prefetch
                    const Win rf = make_win(v.foam + (size_t)ft * TILE, TILE * 4);
#pragma unroll
                    for (int m = 0; m < kElems / RL; ++m)
#pragma unroll
                        for (int q = 0; q < RL; ++q) fb[m * RL + q] = bload1(rf, toff * 4, CT::out_dy(m, q) * W * 4);
                }
                if (more) load(item + gridDim.x, st == 2 ? 1 : 0, nx2);  // next item's R[Q2], R[Q1]
            }
            const Win wd = win16(v.disp, ft);
            [[maybe_unused]] Win wt{};  // (declared between wd and wv: the eager kernels keep their registers)
            if constexpr (!DT) wt = win16(v.turb, ft);
            const Win wv = win16(v.deriv, ft);
            auto emit = [&](int m, int q, float2 val) {
                const int i = m * RL + q;
                const int dy = CT::out_dy(m, q);
                const float s = perm_sign(x0 + lb, lj + dy);
                const float re = val.x * s, im = val.y * s;
                const int so = dy * N * 16;
                if (st == 0) {  // (Dy, Dyx)
                    kput(i, make_float2(re, im));
                } else if (st == 1) {  // (Dx, Dz): DISP
                    const float2 k = kget(i);
                    if constexpr (DC) gstore4(make_float4(re, k.x, im, 1.0f), wd, voff16, so);
                    else gstore4_nt(make_float4(re, k.x, im, 1.0f), wd, voff16, so);
                    kreg[i] = k.y;
                } else if (st == 2) {  // (Dxz, Dzz)
                    kput(i, make_float2(re, im));
                } else {  // (Dyz, Dxx): foam, TURB, DERIV, NORMAL
                    const float2 k = kget(i);  // (Dxz, Dzz)
                    const float f = foam_update(fb[i], im, k.y, k.x);
                    foam[dy * W] = f;
                    if constexpr (!DT) gstore4_nt(make_float4(f, f, f, f), wt, voff16, so);
                    gstore4_nt(make_float4(kreg[i], re, im, k.y), wv, voff16, so);
                    if (v.normals) gstore4_nt(normal_from_deriv(kreg[i], re, im, k.y), win16(v.normal, ft), voff16, so);
                }
            };
            E::run_regs(cur, lds, tws, emit);
            if (st == 0) {
#pragma unroll
                for (int k = 0; k < DPL; ++k)
                    if (k * T + (int)threadIdx.x < N) d0s[k * T + threadIdx.x] = dd[k];
            }
            // ring: after step 1 the formed R[Q4] (nx2) goes first and R[Q3] (nxt) stays next
#pragma unroll
            for (int i = 0; i < kElems; ++i) {
                if (st == 1) {
                    cur[i] = nx2[i];
                } else {
                    cur[i] = nxt[i];
                    nxt[i] = nx2[i];
                }
            }
            __syncthreads();
        }
    }
}
