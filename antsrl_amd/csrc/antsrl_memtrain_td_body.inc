// antsrl_memtrain_td_body.inc — the body of k_mt_td (antsrl_memtrain.hip) and of k_pop_mt_td (antsrl_popmemtrain.hip):
// TD targets, dL/dq and the loss partials, one thread per row.  Name it reads: T (MtTd, this kernel's net and rows).
    __shared__ float red[MT_TD_BLOCK];
    const int b = blockIdx.x * MT_TD_BLOCK + threadIdx.x;
    const int Bp = (T.B + 31) / 32 * 32;
    float contrib = 0.0f;
    if (b < Bp) {
        float dr = 0.0f, dp = 0.0f;
        int ar = -1, ap = -1;
        if (b < T.B) {
            const size_t row = T.idx ? (size_t)T.idx[b] : (size_t)b;
            const int64_t a0 = T.actions[2 * row], a1 = T.actions[2 * row + 1];
            const float rew = T.rewards[row], nd = T.dones[row] ? 0.0f : 1.0f;
            const size_t o = (size_t)b * 32;
            if (a0 >= 0 && a0 < T.n_rot) {
                ar = (int)a0;
                const float y = rew + (T.discount * mt_max(T.tqr + o, T.n_rot)) * nd;
                dr = T.qr[o + ar] - y;
            }
            if (a1 >= 0 && a1 < T.n_ph) {
                ap = (int)a1;
                const float y = rew + (T.discount * mt_max(T.tqp + o, T.n_ph)) * nd;
                dp = T.qp[o + ap] - y;
            }
            contrib = dr * dr * T.inv_r + dp * dp * T.inv_p;
        }
        float4 *gr = reinterpret_cast<float4 *>(T.dqr + (size_t)b * 32), *gp = reinterpret_cast<float4 *>(T.dqp + (size_t)b * 32);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float4 u, v;
            u.x = 4 * c == ar ? dr * T.norm_r : 0.0f; u.y = 4 * c + 1 == ar ? dr * T.norm_r : 0.0f;
            u.z = 4 * c + 2 == ar ? dr * T.norm_r : 0.0f; u.w = 4 * c + 3 == ar ? dr * T.norm_r : 0.0f;
            v.x = 4 * c == ap ? dp * T.norm_p : 0.0f; v.y = 4 * c + 1 == ap ? dp * T.norm_p : 0.0f;
            v.z = 4 * c + 2 == ap ? dp * T.norm_p : 0.0f; v.w = 4 * c + 3 == ap ? dp * T.norm_p : 0.0f;
            gr[c] = u;
            gp[c] = v;
        }
    }
    red[threadIdx.x] = contrib; // fixed-order tree: deterministic
    __syncthreads();
    for (int s = MT_TD_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) T.lossp[blockIdx.x] = red[0];
