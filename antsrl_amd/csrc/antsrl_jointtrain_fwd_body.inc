// antsrl_jointtrain_fwd_body.inc — the body of the forward stage of the joint training step: ONE text, included inside
// the braces of the two kernels that run it, k_jointtrain_fwd (antsrl_jointtrain.hip) and k_pop_jointtrain_fwd
// (antsrl_popjoint.hip).  A textual include and not a __device__ function, for the reason antsrl_policy_flat_body.inc
// gives (DESIGN §7.24): included, k_jointtrain_fwd's text is what it always was.  It reads one name of the including
// kernel: `a`, the L1TrainArgs of the net it trains (its target: layer3), and the x dimension of the grid (the workgroups that share the
// minibatch's tiles).  antsrl_jointtrain.hip's header describes the stage; antsrl_jointtrain_dev.h holds its LDS layout.
    extern __shared__ __align__(16) unsigned char smem[];
    const DqnBatch &mb = a.batch;
    const int F = mb.F, IN = F + 2, ksteps = mb.ksteps, KP = 16 * ksteps + 8; // 8 = bank skew
    __bf16 *w1s = reinterpret_cast<__bf16 *>(smem);                           // [32][KP]: the live W1
    float *hw = reinterpret_cast<float *>(smem + (size_t)JT_HIDDEN * KP * 2); // 3 slots of JT_SLOT: layer2, layer3, the target's layer3
    float *l1x = hw + JT_HW;                                                  // [3][32]: b1 and the bf16-rounded W1 columns F, F + 1
    float *wpart = l1x + 3 * JT_HIDDEN;                                       // [JT_WAVES][JT_PART]
    float *tiles = wpart + JT_WAVES * JT_PART;                                // per wave: h [32][33], dq [32][8]
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wib = threadIdx.x >> 6;
    float *ht = tiles + (size_t)wib * JT_TILE, *dqs = ht + 32 * JT_HSTRIDE;
    const float *b1 = a.model + (size_t)JT_HIDDEN * IN, *heads = b1 + JT_HIDDEN;

    dqn_stage_w1(a.model, w1s, F, ksteps, KP, wib, JT_WAVES, lane);
    for (int i = threadIdx.x; i < JT_HEADS + LT_L3; i += 64 * JT_WAVES)
        hw[(i / LT_L3) * JT_SLOT + i % LT_L3] = i < JT_HEADS ? heads[i] : a.target[i - JT_HEADS];
    if (threadIdx.x < JT_HIDDEN) {
        const int hid = threadIdx.x;
        l1x[hid] = b1[hid];
        l1x[JT_HIDDEN + hid] = dqn_bf16(a.model[(size_t)hid * IN + F]);
        l1x[2 * JT_HIDDEN + hid] = dqn_bf16(a.model[(size_t)hid * IN + F + 1]);
    }
    ht[r * JT_HSTRIDE + 32] = 1.0f; // (both half-waves write the same value)
    __syncthreads();

    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // outputs lane, lane + 64, lane + 128, lane + 192
    // output o as a column of dq times a column of h: w2 [o / 32][o % 32], b2, w3, b3, the loss
    int dcol[4], hcol[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int o = lane + 64 * j;
        if (o < 96) { dcol[j] = o >> 5; hcol[j] = o & 31; }
        else if (o < 99) { dcol[j] = o - 96; hcol[j] = 32; }
        else if (o < 195) { dcol[j] = 3 + ((o - 99) >> 5); hcol[j] = (o - 99) & 31; }
        else if (o < 198) { dcol[j] = 3 + (o - 195); hcol[j] = 32; }
        else { dcol[j] = 6; hcol[j] = 32; } // o == 198: the loss (o > 198 is never stored)
    }

    const int t = blockIdx.x * JT_WAVES + wib; // this wave's tile
    if (t < mb.ntiles) {
        const __bf16 *wrow = w1s + r * KP + 8 * h;
        const int nwhole = F / 16; // k-steps whose 16 inputs all lie inside the row
        const int brow = t * 32 + r;
        const bool valid = brow < mb.B;
        const long long ri = dqn_row(mb, min(brow, mb.B - 1));
        const float *xs = mb.states + (size_t)ri * F, *xn = mb.new_states + (size_t)ri * F;
        f32x16 acc, accn;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] = accn[g] = 0.0f;
        int s = 0;
#pragma unroll 1
        for (; s < nwhole; ++s) {
            const bf16x8 bs = dqn_frag(xs, 16 * s + 8 * h, F, true), bn = dqn_frag(xn, 16 * s + 8 * h, F, true);
            const bf16x8 af = *reinterpret_cast<const bf16x8 *>(wrow + 16 * s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bs, acc, 0, 0, 0);
            accn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bn, accn, 0, 0, 0);
        }
#pragma unroll 1
        for (; s < ksteps; ++s) {
            const bf16x8 bs = dqn_frag(xs, 16 * s + 8 * h, F, false), bn = dqn_frag(xn, 16 * s + 8 * h, F, false);
            const bf16x8 af = *reinterpret_cast<const bf16x8 *>(wrow + 16 * s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bs, acc, 0, 0, 0);
            accn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bn, accn, 0, 0, 0);
        }
        const float as0 = dqn_bf16(mb.agent_states[(size_t)ri * 2]), as1 = dqn_bf16(mb.agent_states[(size_t)ri * 2 + 1]);
        const float an0 = dqn_bf16(mb.new_agent_states[(size_t)ri * 2]), an1 = dqn_bf16(mb.new_agent_states[(size_t)ri * 2 + 1]);
        float hv[16], hn[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) { // accumulator register g = 4 g4 + j of half-wave h is hidden value 8 g4 + 4 h + j
            const float4 bb = *reinterpret_cast<const float4 *>(l1x + 8 * g4 + 4 * h);
            const float4 c0 = *reinterpret_cast<const float4 *>(l1x + JT_HIDDEN + 8 * g4 + 4 * h);
            const float4 c1 = *reinterpret_cast<const float4 *>(l1x + 2 * JT_HIDDEN + 8 * g4 + 4 * h);
            const float bias1[4] = {bb.x, bb.y, bb.z, bb.w}, was0[4] = {c0.x, c0.y, c0.z, c0.w}, was1[4] = {c1.x, c1.y, c1.z, c1.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                hv[4 * g4 + j] = dqn_hidden(acc[4 * g4 + j], as0, was0[j], as1, was1[j], bias1[j]);
                hn[4 * g4 + j] = dqn_hidden(accn[4 * g4 + j], an0, was0[j], an1, was1[j], bias1[j]);
            }
        }
        float qr[3], qp[3], nr[3], np[3];
        // (scheduling fences: the 48 weight vectors of the four heads are not all hoisted in front of the first product)
        __builtin_amdgcn_sched_barrier(0);
        dqn_head(hw, hv, h, qr);                  // model: layer2
        __builtin_amdgcn_sched_barrier(0);
        dqn_head(hw + JT_SLOT, hv, h, qp);        //        layer3
        __builtin_amdgcn_sched_barrier(0);
        dqn_head(hw, hn, h, nr);                  // target: the shared, live layer2
        __builtin_amdgcn_sched_barrier(0);
        dqn_head(hw + 2 * JT_SLOT, hn, h, np);    //         its own layer3
        __builtin_amdgcn_sched_barrier(0);
        const long long ar64 = mb.actions[(size_t)ri * 2], ap64 = mb.actions[(size_t)ri * 2 + 1];
        const int ar = ar64 < 0 ? 0 : (ar64 > 2 ? 2 : (int)ar64), ap = ap64 < 0 ? 0 : (ap64 > 2 ? 2 : (int)ap64);
        const float rew = mb.rewards[ri], live = mb.dones[ri] ? 0.0f : 1.0f;
        const float yr = rew + mb.discount * fmaxf(fmaxf(nr[0], nr[1]), nr[2]) * live;
        const float yp = rew + mb.discount * fmaxf(fmaxf(np[0], np[1]), np[2]) * live;
        const float dr = (ar == 0 ? qr[0] : ar == 1 ? qr[1] : qr[2]) - yr, dp = (ap == 0 ? qp[0] : ap == 1 ? qp[1] : qp[2]) - yp;
        const float gr = valid ? dr * mb.dq_scale : 0.0f, gp = valid ? dp * mb.dq_scale : 0.0f;
#pragma unroll
        for (int g = 0; g < 16; ++g) ht[r * JT_HSTRIDE + (g & 3) + 8 * (g >> 2) + 4 * h] = hv[g];
        if (h == 0) {
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                dqs[r * JT_DSTRIDE + o] = ar == o ? gr : 0.0f;
                dqs[r * JT_DSTRIDE + 3 + o] = ap == o ? gp : 0.0f;
            }
            dqs[r * JT_DSTRIDE + 6] = valid ? dr * dr * mb.loss_scale + dp * dp * mb.loss_scale : 0.0f;
        }
        if (valid) { // dh = dq_rot * w2[a_rot] + dq_ph * w3[a_ph]: the lane's 16 hidden units, four at a time
            float *dst = a.dh + (size_t)brow * JT_HIDDEN;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float4 w2 = *reinterpret_cast<const float4 *>(hw + ar * JT_HIDDEN + 8 * g4 + 4 * h);
                const float4 w3 = *reinterpret_cast<const float4 *>(hw + JT_SLOT + ap * JT_HIDDEN + 8 * g4 + 4 * h);
                *reinterpret_cast<float4 *>(dst + 8 * g4 + 4 * h) =
                    make_float4(gr * w2.x + gp * w3.x, gr * w2.y + gp * w3.y, gr * w2.z + gp * w3.z, gr * w2.w + gp * w3.w);
            }
        }
        dqn_wave_sync();
#pragma unroll 4
        for (int rr = 0; rr < 32; ++rr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] += dqs[rr * JT_DSTRIDE + dcol[j]] * ht[rr * JT_HSTRIDE + hcol[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (lane + 64 * j < JT_OUT) wpart[wib * JT_PART + lane + 64 * j] = out[j];
    __syncthreads();
    if (threadIdx.x < JT_OUT) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < JT_WAVES; ++w) s += wpart[w * JT_PART + threadIdx.x];
        mb.partials[(size_t)blockIdx.x * JT_PART + threadIdx.x] = s;
    }
