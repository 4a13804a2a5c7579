// antsrl_reworktrain_batch_body.inc — the body of k_reworktrain_batch<NQP> (antsrl_reworktrain.hip, whose header has the
// lane layout and the order of every sum) and of k_pop_reworktrain_batch<NQP> (antsrl_poprework.hip).  The including
// kernel names NQP and `a`, the step's ReworkTrainArgs (a member's own, in a population); the body takes its workgroup
// and the number of partials from the x dimension.  Both collapsed buffers are read one float at a time.
    // [NQP][Dp] of the model, [NQP][Dp] of the target (zero rows past NQ, zero columns past D), their biases [2][NQP], then
    // the rows' hand-over [RT_ROWS][RT_INFO]
    extern __shared__ __align__(16) float ws[];
    const int F = a.d.F, D = a.d.D, n_rot = a.d.n_rot, NQ = a.d.n_rot + a.d.n_ph, B = a.B;
    const int nchunks = (D + 63) / 64, Dp = 64 * nchunks, nfull = F / 64;
    float *wm = ws, *wt = ws + NQP * Dp, *bias = ws + 2 * NQP * Dp, *info = bias + 2 * NQP;
    const float *__restrict__ cm = reinterpret_cast<const float *>(a.work + a.L.collapsed), *__restrict__ ct = a.target;
    const int tid = threadIdx.x;
    for (int i = tid; i < NQP * Dp; i += RT_TPB) {
        const int o = i / Dp, k = i - o * Dp;
        const bool in = o < NQ && k < D;
        const size_t src = in ? (size_t)o * D + k : 0; // unconditional loads on a clamped address, then selects
        const float m = cm[src], t = ct[src];
        wm[i] = in ? m : 0.0f;
        wt[i] = in ? t : 0.0f;
    }
    if (tid < 2 * NQP) {
        const int o = tid & (NQP - 1);
        const float v = (tid < NQP ? cm : ct)[(size_t)NQ * D + (o < NQ ? o : 0)];
        bias[tid] = o < NQ ? v : 0.0f;
    }
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, l = lane & 15, r = 4 * (tid >> 6) + g;
    const int npass = (B + RT_ROWS - 1) / RT_ROWS;
    float acc[4][NQP];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < NQP; ++k) acc[j][k] = 0.0f;
    float sacc = 0.0f, lrot = 0.0f, lph = 0.0f;
    for (int pass = blockIdx.x; pass < npass; pass += gridDim.x) {
        {
            const int b = pass * RT_ROWS + r;
            const bool valid = b < B;
            const int bb = valid ? b : B - 1;
            const long long ri = dqn_row(a, bb);
            const float *__restrict__ xs = a.states + (size_t)ri * F, *__restrict__ xn = a.new_states + (size_t)ri * F;
            const float as0 = a.agent_states[(size_t)ri * 2], as1 = a.agent_states[(size_t)ri * 2 + 1];
            const float an0 = a.new_agent_states[(size_t)ri * 2], an1 = a.new_agent_states[(size_t)ri * 2 + 1];
            float q[NQP], qn[NQP];
#pragma unroll
            for (int o = 0; o < NQP; ++o) q[o] = qn[o] = 0.0f;
            for (int c = 0; c < nchunks; ++c) {
                const int k = 64 * c + 4 * l;
                float x[4], y[4];
                if (c < nfull) { // (uniform) the chunk lies inside the observation row
                    const RwF4 vx = *reinterpret_cast<const RwF4 *>(xs + k), vy = *reinterpret_cast<const RwF4 *>(xn + k);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        x[i] = vx.v[i];
                        y[i] = vy.v[i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = min(k + i, F - 1);
                        x[i] = xs[e];
                        y[i] = xn[e];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int kk = k + i;
                        x[i] = kk < F ? x[i] : (kk == F ? as0 : (kk == F + 1 ? as1 : 0.0f));
                        y[i] = kk < F ? y[i] : (kk == F ? an0 : (kk == F + 1 ? an1 : 0.0f));
                    }
                }
#pragma unroll
                for (int o = 0; o < NQP; ++o) {
                    const float4 w = *reinterpret_cast<const float4 *>(wm + o * Dp + k);
                    const float4 v = *reinterpret_cast<const float4 *>(wt + o * Dp + k);
                    q[o] = fmaf(x[0], w.x, q[o]);
                    q[o] = fmaf(x[1], w.y, q[o]);
                    q[o] = fmaf(x[2], w.z, q[o]);
                    q[o] = fmaf(x[3], w.w, q[o]);
                    qn[o] = fmaf(y[0], v.x, qn[o]);
                    qn[o] = fmaf(y[1], v.y, qn[o]);
                    qn[o] = fmaf(y[2], v.z, qn[o]);
                    qn[o] = fmaf(y[3], v.w, qn[o]);
                }
            }
#pragma unroll
            for (int o = 0; o < NQP; ++o) {
                q[o] = rw_group_sum(q[o]) + bias[o];
                qn[o] = rw_group_sum(qn[o]) + bias[NQP + o];
            }
            const long long ar64 = a.actions[(size_t)ri * 2], ap64 = a.actions[(size_t)ri * 2 + 1];
            const int ar = ar64 < 0 ? 0 : (ar64 >= n_rot ? n_rot - 1 : (int)ar64);
            const int apk = n_rot + (ap64 < 0 ? 0 : (ap64 >= a.d.n_ph ? a.d.n_ph - 1 : (int)ap64));
            const float rew = a.rewards[ri], live = a.dones[ri] ? 0.0f : 1.0f;
            float mr = qn[0], mp = 0.0f, qr = q[0], qp = 0.0f;
#pragma unroll
            for (int o = 1; o < NQP; ++o) {
                if (o < n_rot) mr = fmaxf(mr, qn[o]);
                if (o == n_rot) mp = qn[o];
                if (o > n_rot && o < NQ) mp = fmaxf(mp, qn[o]);
            }
#pragma unroll
            for (int o = 0; o < NQP; ++o) {
                qr = o == ar ? q[o] : qr;
                qp = o == apk ? q[o] : qp;
            }
            const float dr = qr - (rew + a.discount * mr * live), dp = qp - (rew + a.discount * mp * live);
            if (l == 0) {
                float *ri_out = info + r * RT_INFO;
                ri_out[0] = valid ? dr * a.dq_rot : 0.0f;
                ri_out[1] = valid ? dp * a.dq_ph : 0.0f;
                ri_out[2] = valid ? dr * dr : 0.0f;
                ri_out[3] = valid ? dp * dp : 0.0f;
                reinterpret_cast<int *>(ri_out)[4] = ar;
                reinterpret_cast<int *>(ri_out)[5] = apk;
                *reinterpret_cast<long long *>(ri_out + 6) = ri;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int rr = 0; rr < RT_ROWS; ++rr) {
            const float *in = info + rr * RT_INFO;
            const float gr = in[0], gp = in[1];
            const int ar = reinterpret_cast<const int *>(in)[4], apk = reinterpret_cast<const int *>(in)[5];
            const size_t ri = (size_t) * reinterpret_cast<const long long *>(in + 6);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (RT_TPB * j < D) { // (uniform)
                    const int c = min(tid + RT_TPB * j, D - 1);
                    const float xo = a.states[ri * F + min(c, F - 1)], xa = a.agent_states[ri * 2 + max(c - F, 0)];
                    const float x = c < F ? xo : xa;
                    const float tr = gr * x, tp = gp * x;
#pragma unroll
                    for (int k = 0; k < NQP; ++k) acc[j][k] = acc[j][k] + (k == ar ? tr : (k == apk ? tp : 0.0f));
                }
            }
            sacc = sacc + (tid == ar ? gr : (tid == apk ? gp : 0.0f));
            lrot = lrot + in[2];
            lph = lph + in[3];
        }
        __syncthreads(); // the hand-over is free for the next rows
    }
    float *part = reinterpret_cast<float *>(a.work + a.L.partials) + (size_t)blockIdx.x * a.L.part_stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = tid + RT_TPB * j;
        if (c < D) {
#pragma unroll
            for (int k = 0; k < NQP; ++k)
                if (k < NQ) part[(size_t)k * D + c] = acc[j][k];
        }
    }
    if (tid < NQ) part[(size_t)NQ * D + tid] = sacc;
    if (tid == 64) {
        part[(size_t)NQ * D + NQ] = lrot;
        part[(size_t)NQ * D + NQ + 1] = lph;
    }
