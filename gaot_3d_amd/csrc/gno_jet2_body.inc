// The body of the two directional 2-jet kernels of gno_jet2.hip, included once in each: k_gno_fwd_knn_jet2 (regular lists, R = false)
// and k_gno_fwd_rows_jet2 (ragged rows, R = true).  Textual inclusion, not a shared __device__ function: inlined from a function the
// regular-list kernels load their by-value arguments at other places and come out with other instruction streams; as statements of
// the kernel itself they are the kernels they were.  In scope: NH, MODE, R, the kernel's arguments mlp, y_pos, x_pos, f_y, ttab, nbr,
// lk, E, dirs, out, d1, d2 and a Jet2Rows `rows` (read only where R), and QD: false with `dirs` a by-value Jet2Dirs, true in the two
// per-query kernels k_gno_qd_jet2_knn / k_gno_qd_jet2_rows, where `dirs` is a Jet2QDirs and the direction of a lane is that of its
// edge's query.
    using L = Jet2Lds<NH>;
    constexpr bool KEEP = NH <= 2;   // what the value path leaves for the direction passes (see the head of this file)
    extern __shared__ __attribute__((aligned(16))) float lds[];

    // ---- weights -> LDS, transposed to [in][out] (k_gno_fwd's image) ---------------------------------
    for (int i = threadIdx.x; i < IN0P * H; i += 256) {
        const int k = i / H, j = i % H;
        lds[L::w0 + i] = (k < IN0) ? mlp.w[0][j * IN0 + k] : 0.f;
    }
    for (int i = threadIdx.x; i < H; i += 256) lds[L::b0 + i] = mlp.b[0][i];
#pragma unroll
    for (int l = 1; l < NH; ++l) {
        float* wt = lds + L::wl + (l - 1) * (H * H + H);
        for (int i = threadIdx.x; i < H * H; i += 256) {
            const int j = i / H, k = i % H;
            wt[k * H + j] = mlp.w[l][i];
        }
        for (int i = threadIdx.x; i < H; i += 256) wt[H * H + i] = mlp.b[l][i];
    }
    for (int i = threadIdx.x; i < C * H; i += 256) {
        const int c = i / H, k = i % H;
        lds[L::wL + k * C + c] = mlp.w[NH][i];
    }
    for (int i = threadIdx.x; i < C; i += 256) lds[L::bL + i] = mlp.b[NH][i];
    __syncthreads();

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, hf = lane >> 5;
    float* stage = lds + L::stage + wave * (2 * 32 * C);
    int* ids = (int*)(lds + L::ids) + wave * 32;
    int64_t plane;                         // one [Nq][32] plane of d1 / d2
    [[maybe_unused]] int* qids = nullptr;
    if constexpr (R) {
        plane = rows.plane;
        qids = (int*)(lds + L::qids) + wave * 32;
    } else {
        plane = (E >> lk) * C;
    }

    const int64_t n_tiles = (E + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t base = tile * 32;
        // MLP input k = 2i+hf of this lane's edge: [y.x y.y y.z x.x x.y x.z][2i+hf], i = 0..2 (edges past E: row 0, a valid row)
        float bin[3];
        int sid;
        {
            const int64_t e = base + l31;
            const bool valid = e < E;
            sid = valid ? nbr[e] : 0;
            int q;
            [[maybe_unused]] int qid = -1;   // row lists: the edge's row; -1 = no row (past E, or a padding edge of the list)
            if constexpr (R) {
                if (valid) qid = rows.dst_s[e];
                q = qid < 0 ? 0 : qid;       // a valid row to read coordinates from
            } else {
                q = valid ? (int)(e >> lk) : 0;
            }
            const float* ys = y_pos + (int64_t)sid * 3;
            const float* xq = x_pos + (int64_t)q * 3;
            bin[0] = ys[hf];
            bin[1] = hf ? xq[0] : ys[2];
            bin[2] = xq[1 + hf];
            if (hf == 0) {
                ids[l31] = sid;
                if constexpr (R) qids[l31] = qid;
            }
        }
        // ---- the value path, once per tile: gelu' and gelu'' of every hidden layer stay in registers -----
        f32x16 h[KB], sa[NH][KB], sb[KEEP ? NH : 1][KB];   // KEEP: gelu'(z_l), gelu''(z_l); else z_l
#pragma unroll
        for (int ob = 0; ob < KB; ++ob) {
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = lds[L::b0 + 32 * ob + mfma32_row(r, hf)];
            if constexpr (MODE != MODE_LINEAR) {
                const float* tr = ttab + (int64_t)sid * NLH + 32 * ob + 4 * hf;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 v = *reinterpret_cast<const float4*>(tr + 8 * j);
                    z[4 * j + 0] += v.x;
                    z[4 * j + 1] += v.y;
                    z[4 * j + 2] += v.z;
                    z[4 * j + 3] += v.w;
                }
            }
#pragma unroll
            for (int i = 0; i < IN0 / 2; ++i) {
                const float a = lds[L::w0 + (2 * i + hf) * H + 32 * ob + l31];
                z = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bin[i], z, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float g, a, b;
                gelu_fast_jet2(z[r], g, a, b);
                h[ob][r] = g;
                if constexpr (KEEP) {
                    sa[0][ob][r] = a;
                    sb[0][ob][r] = b;
                } else {
                    sa[0][ob][r] = z[r];
                }
            }
        }
#pragma unroll
        for (int l = 1; l < NH; ++l) {
            const float* wt = lds + L::wl + (l - 1) * (H * H + H);
            f32x16 zn[KB];
#pragma unroll
            for (int ob = 0; ob < KB; ++ob) {
#pragma unroll
                for (int r = 0; r < 16; ++r) zn[ob][r] = wt[H * H + 32 * ob + mfma32_row(r, hf)];
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float a = wt[(32 * kb + mfma32_row(r, hf)) * H + 32 * ob + l31];
                        zn[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, h[kb][r], zn[ob], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float g, a, b;
                    gelu_fast_jet2(zn[ob][r], g, a, b);
                    h[ob][r] = g;
                    if constexpr (KEEP) {
                        sa[l][ob][r] = a;
                        sb[l][ob][r] = b;
                    } else {
                        sa[l][ob][r] = zn[ob][r];
                    }
                }
        }
        // ---- last layer, transposed: K'[e][c] = sum_k Hlast[k][e] * WL[c][k] + bL[c]; the value plane is finished by half 0 ----
        wave_lds_fence();  // ids visible to the whole wave
        [[maybe_unused]] float fv[16];
        if constexpr (MODE != MODE_KERNELONLY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) fv[r] = f_y[(int64_t)ids[mfma32_row(r, hf)] * C + l31];
        }
        {
            f32x16 acc;
            const float bl = lds[L::bL + l31];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = bl;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float b = lds[L::wL + (32 * kb + mfma32_row(r, hf)) * C + l31];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h[kb][r], b, acc, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int el = mfma32_row(r, hf);
                if constexpr (MODE == MODE_KERNELONLY) stage[el * C + l31] = acc[r];
                else stage[el * C + l31] = acc[r] * fv[r];
            }
        }
        wave_lds_fence();
        if (hf == 0) {
            if constexpr (R)
                segment_walk<C>(stage, C, qids, l31, base, rows.rowptr, out, rows.part, true);
            else
                fixed_k_rows<C>(stage, C, l31, base, lk, E, out);
        }
        wave_lds_fence();

        // ---- one pass per direction: h' and h'' through the layers, two planes staged, one finished by each half ----
#pragma unroll 1
        for (int d = 0; d < dirs.nd; ++d) {
            float vx, vy, vz;
            if constexpr (QD) {
                // the lane's edge is base + l31 in both halves; its query is found again here (an LDS word / a shift), so that no
                // register is held across the value path and the layer loops: query 0 for edges past E and padding edges
                int q;
                if constexpr (R) {
                    q = qids[l31];
                    q = q < 0 ? 0 : q;
                } else {
                    q = base + l31 < E ? (int)((base + l31) >> lk) : 0;
                }
                const float* v = qdir_at(dirs, ((int64_t)q * dirs.nd + d) * 3);
                vx = v[0];
                vy = v[1];
                vz = v[2];
            } else {
                vx = dir_at(dirs, d, 0);
                vy = dir_at(dirs, d, 1);
                vz = dir_at(dirs, d, 2);
            }
            f32x16 hd[KB], hdd[KB];
#pragma unroll
            for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = 32 * ob + mfma32_row(r, hf);
                    const float zd = fmaf(vz, lds[L::w0 + 5 * H + j], fmaf(vy, lds[L::w0 + 4 * H + j], vx * lds[L::w0 + 3 * H + j]));
                    float dg, ddg;
                    if constexpr (KEEP) {
                        dg = sa[0][ob][r];
                        ddg = sb[0][ob][r];
                    } else {
                        float g;
                        gelu_fast_jet2(opaque(sa[0][ob][r]), g, dg, ddg);
                    }
                    hd[ob][r] = dg * zd;
                    hdd[ob][r] = ddg * zd * zd;
                }
#pragma unroll
            for (int l = 1; l < NH; ++l) {
                const float* wt = lds + L::wl + (l - 1) * (H * H + H);
                f32x16 u[KB], w[KB];
#pragma unroll
                for (int ob = 0; ob < KB; ++ob) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) u[ob][r] = 0.f;
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float a = wt[(32 * kb + mfma32_row(r, hf)) * H + 32 * ob + l31];
                            u[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, hd[kb][r], u[ob], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int ob = 0; ob < KB; ++ob) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) w[ob][r] = 0.f;
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float a = wt[(32 * kb + mfma32_row(r, hf)) * H + 32 * ob + l31];
                            w[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, hdd[kb][r], w[ob], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float dg, ddg;
                        if constexpr (KEEP) {
                            dg = sa[l][ob][r];
                            ddg = sb[l][ob][r];
                        } else {
                            float g;
                            gelu_fast_jet2(opaque(sa[l][ob][r]), g, dg, ddg);
                        }
                        hd[ob][r] = dg * u[ob][r];
                        hdd[ob][r] = fmaf(dg, w[ob][r], ddg * u[ob][r] * u[ob][r]);
                    }
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float b = lds[L::wL + (32 * kb + mfma32_row(r, hf)) * C + l31];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p == 0 ? hd[kb][r] : hdd[kb][r], b, acc, 0, 0, 0);
                    }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int el = mfma32_row(r, hf);
                    if constexpr (MODE == MODE_KERNELONLY) stage[(p * 32 + el) * C + l31] = acc[r];
                    else stage[(p * 32 + el) * C + l31] = acc[r] * fv[r];
                }
            }
            wave_lds_fence();
            if constexpr (R)
                segment_walk<C>(stage + hf * 32 * C, C, qids, l31, base, rows.rowptr, (hf ? d2 : d1) + (int64_t)d * plane,
                                rows.part + (1 + (hf ? dirs.nd : 0) + d) * rows.part_plane, true);
            else
                fixed_k_rows<C>(stage + hf * 32 * C, C, l31, base, lk, E, (hf ? d2 : d1) + (int64_t)d * plane);
            wave_lds_fence();
        }
    }
