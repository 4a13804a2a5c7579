// antsrl_rework_act_body.inc — the body of k_rework_act<OBS16, NQP, SEL> (antsrl_rework.hip, whose header has the lane
// layout, the order of a row's sums and the three kinds of pass) and of k_pop_rework_act<OBS16, NQP, SEL>
// (antsrl_poprework.hip).  The including kernel names the template parameters and `collapsed`, `obs_`, `agent_state`,
// `rot_out`, `ph_out`, `q_out`, `M`, `F`, `n_rot`, `n_ph`, `nchunks` and `sel` (read with SEL only); the body takes its
// workgroup and the grid's width from the x dimension.  Rows past M are clamped to row M - 1 and not written; the bf16
// path's last_dword is that of the M rows behind `obs_`.
    // Wc in LDS, zero rows past NQ, zero columns past D, in the order a lane reads it: [output pair p][chunk c][half h]
    // [lane l][4] with the four floats Wc[2p][k], Wc[2p+1][k], Wc[2p][k+1], Wc[2p+1][k+1] at k = 64 c + 4 l + 2 h
    extern __shared__ __align__(16) float ws[];
    const int D = F + 2, NQ = n_rot + n_ph, Dp = 64 * nchunks;
    for (int idx = threadIdx.x; idx < NQP * Dp; idx += RW_TPB) {
        const int p = idx / (2 * Dp), r = idx - p * (2 * Dp), c = r >> 7, h = (r >> 6) & 1, l = (r >> 2) & 15, e = r & 3;
        const int o = 2 * p + (e & 1), k = 64 * c + 4 * l + 2 * h + (e >> 1);
        const bool in = o < NQ && k < D;
        const float w = collapsed[in ? (size_t)o * D + k : 0]; // unconditional load on a clamped address, then select
        ws[idx] = in ? w : 0.0f;
    }
    __syncthreads();

    const float *obs = static_cast<const float *>(obs_);
    const uint16_t *obs16 = static_cast<const uint16_t *>(obs_);
    const uint32_t *obs32 = static_cast<const uint32_t *>(obs_);
    const size_t last_dword = (size_t)M * F / 2 - 1; // bf16: the buffer's last whole dword (used by full chunks: F >= 64)
    const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15;
    const int wave = (blockIdx.x * RW_TPB + threadIdx.x) >> 6, nwaves = (gridDim.x * RW_TPB) >> 6;
    const int nfull = F / 64;                  // chunks that lie inside the observation row
    const int npass = (int)(((long long)M + 4 * RW_U - 1) / (4 * RW_U));
    float bias[NQP];
#pragma unroll
    for (int o = 0; o < NQP; ++o) bias[o] = collapsed[(size_t)NQ * D + (o < NQ ? o : 0)];
    // (SEL: the pass index in a scalar register, so that a pass inside one colony keeps its explore draw on the scalar unit)
    for (int pass = SEL ? __builtin_amdgcn_readfirstlane(wave) : wave; pass < npass; pass += nwaves) {
        // SEL: lane j < 4 RW_U looks after row `first + j` of the pass: its colony `env`, its ant index `ant` there, and
        // `key`, the two rounds every draw of that colony at this step starts with.  `ex` and `rows` are wave-uniform.
        uint32_t ex = 0;   // bit j: row first + j belongs to a colony that explores this step
        uint32_t rows = 0; // bit j: row first + j lies inside the batch
        if (SEL) {
            uint32_t env, ant;
            uint64_t key;
            const uint32_t first = (uint32_t)pass * (4 * RW_U), valid = min((uint32_t)(4 * RW_U), (uint32_t)M - first);
            const uint32_t e0 = first / sel.n_ants, a0 = first - e0 * sel.n_ants;
            rows = (1u << valid) - 1u;
            if (a0 + valid <= sel.n_ants) { // the pass lies inside one colony: one draw, on wave-uniform values
                env = e0;
                ant = a0 + (uint32_t)(lane & (4 * RW_U - 1));
                key = draw_env_step(sel.seed, (uint64_t)sel.env_base + e0, sel.step);
                ex = draw_u01(draw_item(key, 0, ANTSRL_DRAW_EXPLORE)) < sel.epsilon ? rows : 0u;
            } else { // it straddles colonies: one draw per row, lanes past the batch on its last row (masked by `rows`)
                const uint32_t r = min(first + (uint32_t)(lane & (4 * RW_U - 1)), (uint32_t)M - 1u);
                env = r / sel.n_ants;
                ant = r - env * sel.n_ants;
                key = draw_env_step(sel.seed, (uint64_t)sel.env_base + env, sel.step);
                ex = (uint32_t)__ballot(draw_u01(draw_item(key, 0, ANTSRL_DRAW_EXPLORE)) < sel.epsilon) & rows;
            }
            // the drawn actions, by the row's lane alone, and in front of the evaluation, across which only `ex` then lives
            if (ex != 0 && lane < 4 * RW_U && ((ex >> lane) & 1u)) {
                const size_t row = (size_t)first + lane;
                rot_out[row] = (int8_t)((int)draw_below(draw_item(key, ant, ANTSRL_DRAW_ROTATION), (uint32_t)n_rot) - n_rot / 2);
                ph_out[row] = (int8_t)draw_below(draw_item(key, ant, ANTSRL_DRAW_PHEROMONE), (uint32_t)n_ph);
            }
            // a colony's flag is written by the lane of its first ant's row: one writer
            if (sel.explored && lane < 4 * RW_U && ((rows >> lane) & 1u) && ant == 0) sel.explored[env] = (uint8_t)((ex >> lane) & 1u);
        }
        if (!SEL || ex != rows) { // (wave-uniform) a pass whose rows all explore loads nothing and multiplies nothing
            long long m[RW_U];
            size_t base[RW_U]; // element index of the row's start, the row clamped into the batch
            float as0[RW_U], as1[RW_U];
#pragma unroll
            for (int u = 0; u < RW_U; ++u) {
                m[u] = (long long)pass * (4 * RW_U) + 4 * u + g;
                const size_t mc = (size_t)(m[u] < M ? m[u] : M - 1);
                base[u] = mc * F;
                as0[u] = agent_state[mc * 2];
                as1[u] = agent_state[mc * 2 + 1];
            }
            rw_f32x2 acc[RW_U][NQP / 2]; // outputs 2 p and 2 p + 1: one packed fma for both
#pragma unroll
            for (int u = 0; u < RW_U; ++u)
#pragma unroll
                for (int p = 0; p < NQP / 2; ++p) acc[u][p] = rw_f32x2{0.0f, 0.0f};
            // a chunk inside the observation row: one wide load per row (bf16: three aligned dwords and a funnel shift)
            auto load_full = [&](int c, float(&x)[RW_U][4]) {
                const int k = 64 * c + 4 * l;
#pragma unroll
                for (int u = 0; u < RW_U; ++u) {
                    if (OBS16) {
                        const size_t e = base[u] + k, d0 = e >> 1;
                        const size_t d2 = d0 + 2 < last_dword ? d0 + 2 : last_dword;
                        const uint32_t w0 = obs32[d0], w1 = obs32[d0 + 1], w2 = obs32[d2];
                        const uint32_t sh = (uint32_t)(e & 1) * 16u;
                        const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh), hi = __builtin_amdgcn_alignbit(w2, w1, sh);
                        x[u][0] = __uint_as_float(lo << 16);
                        x[u][1] = __uint_as_float(lo & 0xffff0000u);
                        x[u][2] = __uint_as_float(hi << 16);
                        x[u][3] = __uint_as_float(hi & 0xffff0000u);
                    } else {
                        const RwF4 v = *reinterpret_cast<const RwF4 *>(obs + base[u] + k);
#pragma unroll
                        for (int i = 0; i < 4; ++i) x[u][i] = v.v[i];
                    }
                }
            };
            // the row's end, agent_state, the zero pad: loads on addresses clamped into the row, then selects
            // (every load unconditional: inside a per-lane branch each one gets its own s_waitcnt vmcnt(0))
            auto load_tail = [&](int c, float(&x)[RW_U][4]) {
                const int k = 64 * c + 4 * l;
#pragma unroll
                for (int u = 0; u < RW_U; ++u)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const size_t e = base[u] + min(k + i, F - 1);
                        x[u][i] = OBS16 ? __uint_as_float((uint32_t)obs16[e] << 16) : obs[e];
                    }
#pragma unroll
                for (int u = 0; u < RW_U; ++u)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int kk = k + i;
                        x[u][i] = kk < F ? x[u][i] : (kk == F ? as0[u] : (kk == F + 1 ? as1[u] : 0.0f));
                    }
            };
            auto mac = [&](int c, const float(&x)[RW_U][4]) {
#pragma unroll
                for (int p = 0; p < NQP / 2; ++p) {
                    const float *wp = ws + ((p * nchunks + c) * 2) * 64 + 4 * l;
                    const float4 wa = *reinterpret_cast<const float4 *>(wp), wb = *reinterpret_cast<const float4 *>(wp + 64);
#pragma unroll
                    for (int u = 0; u < RW_U; ++u) {
                        acc[u][p] = __builtin_elementwise_fma(rw_f32x2{x[u][0], x[u][0]}, rw_f32x2{wa.x, wa.y}, acc[u][p]);
                        acc[u][p] = __builtin_elementwise_fma(rw_f32x2{x[u][1], x[u][1]}, rw_f32x2{wa.z, wa.w}, acc[u][p]);
                        acc[u][p] = __builtin_elementwise_fma(rw_f32x2{x[u][2], x[u][2]}, rw_f32x2{wb.x, wb.y}, acc[u][p]);
                        acc[u][p] = __builtin_elementwise_fma(rw_f32x2{x[u][3], x[u][3]}, rw_f32x2{wb.z, wb.w}, acc[u][p]);
                    }
                }
            };
            // the loads of RW_G chunks are issued before the first of them is used: a wave keeps RW_G * RW_U wide loads in
            // flight (one chunk at a time: float32 rows 0.069 ms instead of 0.057 at 512 x 512 rows of 294; DESIGN 7.14)
            int c = 0;
            for (; c + RW_G <= nfull; c += RW_G) {
                float x[RW_G][RW_U][4];
#pragma unroll
                for (int j = 0; j < RW_G; ++j) load_full(c + j, x[j]);
#pragma unroll
                for (int j = 0; j < RW_G; ++j) mac(c + j, x[j]);
            }
            for (; c < nchunks; ++c) {
                float x[RW_U][4];
                if (c < nfull)
                    load_full(c, x);
                else
                    load_tail(c, x);
                mac(c, x);
            }
#pragma unroll
            for (int u = 0; u < RW_U; ++u) {
                float q[NQP];
#pragma unroll
                for (int o = 0; o < NQP; ++o) q[o] = rw_group_sum(acc[u][o >> 1][o & 1]) + bias[o];
                // first maximum of each head (a NaN never wins)
                int ir = 0, ip = 0;
                float br = q[0], bp = 0.0f;
#pragma unroll
                for (int o = 1; o < NQP; ++o) {
                    if (o < n_rot && q[o] > br) {
                        br = q[o];
                        ir = o;
                    }
                    if (o == n_rot) bp = q[o];
                    if (o > n_rot && o < NQ && q[o] > bp) {
                        bp = q[o];
                        ip = o - n_rot;
                    }
                }
                // (SEL: an exploring row of a mixed pass was evaluated like the others and is not stored from here)
                if (l == 0 && m[u] < M && !(SEL && ((ex >> (4 * u + g)) & 1u))) {
                    rot_out[m[u]] = (int8_t)(ir - n_rot / 2);
                    ph_out[m[u]] = (int8_t)ip;
                    if (q_out) {
#pragma unroll
                        for (int o = 0; o < NQP; ++o)
                            if (o < NQ) q_out[(size_t)m[u] * NQ + o] = q[o];
                    }
                }
            }
        }
    }
