// antsrl_exptrain_fwd_body.inc — the body of the forward stage of the explore agent's training step: ONE text, included
// inside the braces of the two kernels that run it, k_exptrain_fwd (antsrl_exptrain.hip) and k_pop_exptrain_fwd
// (antsrl_popexplore.hip).  A textual include and not a __device__ function, for the reason antsrl_policy_flat_body.inc
// gives (DESIGN §7.24): included, k_exptrain_fwd's text is what it always was.  It reads one name of the including
// kernel: `a`, the L1TrainArgs of the net it trains, and the x dimension of the grid (the workgroups that share the
// minibatch's tiles).  antsrl_exptrain.hip's header describes the stage; antsrl_exptrain_dev.h holds its LDS layout.
    extern __shared__ __align__(16) unsigned char smem[];
    const DqnBatch &mb = a.batch;
    const int F = mb.F, IN = F + 2, ksteps = mb.ksteps, KP = 16 * ksteps + 8; // 8 = bank skew
    __bf16 *w1s = reinterpret_cast<__bf16 *>(smem);                  // [2][32][KP]: the model's W1, the target's
    float *hw = reinterpret_cast<float *>(smem + (size_t)2 * ET_HIDDEN * KP * 2); // 2 slots of ET_SLOT: layer2 of the model, of the target
    float *l1x = hw + 2 * ET_SLOT;                                   // [2][3][32]: b1 and the bf16-rounded W1 columns F, F + 1
    float *wpart = l1x + 6 * ET_HIDDEN;                              // [ET_WAVES][ET_PART]
    float *tiles = wpart + ET_WAVES * ET_PART;                       // per wave: h [32][33], dq [32][4]
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wib = threadIdx.x >> 6;
    float *ht = tiles + (size_t)wib * ET_TILE, *dqs = ht + 32 * ET_HSTRIDE;
    const size_t ob1 = (size_t)ET_HIDDEN * IN, ol2 = ob1 + ET_HIDDEN;

    for (int net = 0; net < 2; ++net) {
        const float *blk = net ? a.target : a.model;
        dqn_stage_w1(blk, w1s + net * ET_HIDDEN * KP, F, ksteps, KP, wib, ET_WAVES, lane);
        for (int i = threadIdx.x; i < ET_L2; i += 64 * ET_WAVES) hw[net * ET_SLOT + i] = blk[ol2 + i];
        if (threadIdx.x < ET_HIDDEN) {
            const int hid = threadIdx.x;
            l1x[(3 * net) * ET_HIDDEN + hid] = blk[ob1 + hid];
            l1x[(3 * net + 1) * ET_HIDDEN + hid] = et_bf16(blk[(size_t)hid * IN + F]);
            l1x[(3 * net + 2) * ET_HIDDEN + hid] = et_bf16(blk[(size_t)hid * IN + F + 1]);
        }
    }
    ht[r * ET_HSTRIDE + 32] = 1.0f; // (both half-waves write the same value)
    __syncthreads();

    float out[2] = {0.0f, 0.0f}; // outputs lane, lane + 64: w2 [o / 32][o % 32], b2, the loss
    int dcol[2], hcol[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int o = lane + 64 * j;
        if (o < 96) { dcol[j] = o >> 5; hcol[j] = o & 31; }
        else if (o < 99) { dcol[j] = o - 96; hcol[j] = 32; }
        else { dcol[j] = 3; hcol[j] = 32; } // o == 99: the loss (o > 99 is never stored)
    }

    const int t = blockIdx.x * ET_WAVES + wib; // this wave's tile
    if (t < mb.ntiles) {
        const __bf16 *wrow = w1s + r * KP + 8 * h, *wrow_t = wrow + ET_HIDDEN * KP;
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
            const bf16x8 am = *reinterpret_cast<const bf16x8 *>(wrow + 16 * s), at = *reinterpret_cast<const bf16x8 *>(wrow_t + 16 * s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bs, acc, 0, 0, 0);
            accn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at, bn, accn, 0, 0, 0);
        }
#pragma unroll 1
        for (; s < ksteps; ++s) {
            const bf16x8 bs = dqn_frag(xs, 16 * s + 8 * h, F, false), bn = dqn_frag(xn, 16 * s + 8 * h, F, false);
            const bf16x8 am = *reinterpret_cast<const bf16x8 *>(wrow + 16 * s), at = *reinterpret_cast<const bf16x8 *>(wrow_t + 16 * s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bs, acc, 0, 0, 0);
            accn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at, bn, accn, 0, 0, 0);
        }
        const float as0 = et_bf16(mb.agent_states[(size_t)ri * 2]), as1 = et_bf16(mb.agent_states[(size_t)ri * 2 + 1]);
        const float an0 = et_bf16(mb.new_agent_states[(size_t)ri * 2]), an1 = et_bf16(mb.new_agent_states[(size_t)ri * 2 + 1]);
        float hv[16], hn[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) { // accumulator register g = 4 g4 + j of half-wave h is hidden value 8 g4 + 4 h + j
            const int o = 8 * g4 + 4 * h;
            const float4 bb = *reinterpret_cast<const float4 *>(l1x + o);
            const float4 c0 = *reinterpret_cast<const float4 *>(l1x + ET_HIDDEN + o);
            const float4 c1 = *reinterpret_cast<const float4 *>(l1x + 2 * ET_HIDDEN + o);
            const float4 tb = *reinterpret_cast<const float4 *>(l1x + 3 * ET_HIDDEN + o);
            const float4 t0 = *reinterpret_cast<const float4 *>(l1x + 4 * ET_HIDDEN + o);
            const float4 t1 = *reinterpret_cast<const float4 *>(l1x + 5 * ET_HIDDEN + o);
            const float bm[4] = {bb.x, bb.y, bb.z, bb.w}, m0[4] = {c0.x, c0.y, c0.z, c0.w}, m1[4] = {c1.x, c1.y, c1.z, c1.w};
            const float bt[4] = {tb.x, tb.y, tb.z, tb.w}, u0[4] = {t0.x, t0.y, t0.z, t0.w}, u1[4] = {t1.x, t1.y, t1.z, t1.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                hv[4 * g4 + j] = dqn_hidden(acc[4 * g4 + j], as0, m0[j], as1, m1[j], bm[j]);
                hn[4 * g4 + j] = dqn_hidden(accn[4 * g4 + j], an0, u0[j], an1, u1[j], bt[j]);
            }
        }
        float q[3], qn[3];
        __builtin_amdgcn_sched_barrier(0); // (the weight vectors of both heads are not all hoisted in front of the first product)
        dqn_head(hw, hv, h, q);             // the model's layer2 on h
        __builtin_amdgcn_sched_barrier(0);
        dqn_head(hw + ET_SLOT, hn, h, qn);  // the target's on h'
        __builtin_amdgcn_sched_barrier(0);
        const long long a64 = mb.actions[(size_t)ri * 2];
        const int act = a64 < 0 ? 0 : (a64 > 2 ? 2 : (int)a64);
        const float live = mb.dones[ri] ? 0.0f : 1.0f;
        const float y = mb.rewards[ri] + mb.discount * fmaxf(fmaxf(qn[0], qn[1]), qn[2]) * live;
        const float d = (act == 0 ? q[0] : act == 1 ? q[1] : q[2]) - y;
        const float gq = valid ? d * mb.dq_scale : 0.0f;
#pragma unroll
        for (int g = 0; g < 16; ++g) ht[r * ET_HSTRIDE + (g & 3) + 8 * (g >> 2) + 4 * h] = hv[g];
        if (h == 0) {
#pragma unroll
            for (int o = 0; o < 3; ++o) dqs[r * ET_DSTRIDE + o] = act == o ? gq : 0.0f;
            dqs[r * ET_DSTRIDE + 3] = valid ? d * d * mb.loss_scale : 0.0f;
        }
        if (valid) { // dh = dq * w2[a]: the lane's 16 hidden units, four at a time
            float *dst = a.dh + (size_t)brow * ET_HIDDEN;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float4 ww = *reinterpret_cast<const float4 *>(hw + act * ET_HIDDEN + 8 * g4 + 4 * h);
                *reinterpret_cast<float4 *>(dst + 8 * g4 + 4 * h) = make_float4(gq * ww.x, gq * ww.y, gq * ww.z, gq * ww.w);
            }
        }
        dqn_wave_sync();
#pragma unroll 4
        for (int rr = 0; rr < 32; ++rr) {
#pragma unroll
            for (int j = 0; j < 2; ++j) out[j] += dqs[rr * ET_DSTRIDE + dcol[j]] * ht[rr * ET_HSTRIDE + hcol[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (lane + 64 * j < ET_OUT) wpart[wib * ET_PART + lane + 64 * j] = out[j];
    __syncthreads();
    if (threadIdx.x < ET_OUT) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < ET_WAVES; ++w) s += wpart[w * ET_PART + threadIdx.x];
        mb.partials[(size_t)blockIdx.x * ET_PART + threadIdx.x] = s;
    }
