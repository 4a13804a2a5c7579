// antsrl_replay_record_body.inc — the body of k_replay_record, ONE text included inside k_replay_record
// (antsrl_memagent.hip) and k_pop_record (antsrl_population.hip); see antsrl_policy_flat_body.inc for why it is an include.
// One wave per replay entry: wave (threadIdx.x >> 6) of workgroup blockIdx.x writes entry 4 * blockIdx.x + wave.  Reads the
// including kernel's `a` (RecArgs) and its template flags BF16 and POST; it may return, so it stands last in its kernel.
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= a.n_write) return;
    const long long j = a.j0 + w;
    long long row = a.row0 + w;
    if (row >= a.max_len) row -= a.max_len;
    long long ant = j; // K == M: the identity
    if (a.K != a.M) {
        const long long lo = j * a.M / a.K, hi = (j + 1) * a.M / a.K, n = hi - lo;
        long long off = 0;
        if (n > 1) {
            const double u = draw_u01(agent_draw(a.seed, ANTSRL_DRAW_SAMPLE, a.env_base, a.step, (uint64_t)j));
            off = (long long)floor(u * (double)n);
            if (off > n - 1) off = n - 1;
        }
        ant = lo + off;
    }

    // ---- the observation row
    const int F = a.F;
    const size_t esz = BF16 ? 2 : 4;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(a.obs) + (size_t)ant * (size_t)a.pitch * esz;
    float *dst = a.states + (size_t)row * F;
    int h = (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2); // elements in front of dst's first 16-byte boundary
    if (h > F) h = F;
    const int nvec = (F - h) >> 2, t0 = h + 4 * nvec;
    if (lane < h)
        dst[lane] = load1<BF16>(src, lane);
    else if (t0 + (lane - h) < F)
        dst[t0 + (lane - h)] = load1<BF16>(src, t0 + (lane - h));
    const unsigned char *sb = src + (size_t)h * esz;
    const uintptr_t sa = (uintptr_t)sb;
    const int mode = BF16 ? ((sa & 7) == 0 ? 0 : (sa & 3) == 0 ? 1 : 2) : ((sa & 15) == 0 ? 0 : (sa & 7) == 0 ? 1 : 2);
    float4 *dv = reinterpret_cast<float4 *>(dst + h);
    for (int v = lane; v < nvec; v += 128) { // two rounds of loads in flight before the stores
        const bool two = v + 64 < nvec;
        const float4 x0 = load4<BF16>(sb + (size_t)v * 4 * esz, mode);
        float4 x1 = x0;
        if (two) x1 = load4<BF16>(sb + (size_t)(v + 64) * 4 * esz, mode);
        store_stream(&dv[v], x0);
        if (two) store_stream(&dv[v + 64], x1);
    }

    // ---- the small fields, on the highest lanes
    const int c = 63 - lane, AM = a.A + a.mem;
    if (c < AM)
        a.agent_states[(size_t)row * AM + c] = c < a.A ? a.agent_state[(size_t)ant * a.A + c] : a.memory[(size_t)ant * a.mem + (c - a.A)];
    if (POST) {
        if (c == 0) a.rewards[row] = a.reward[ant];
        if (c == 1) a.dones[row] = a.done[(uint32_t)ant / (uint32_t)a.n_ants] ? 1 : 0;
    } else {
        if (c == 0) a.actions[2 * row] = (int64_t)a.rot[ant] + a.half_rot;
        if (c == 1) a.actions[2 * row + 1] = a.ph ? (int64_t)a.ph[ant] : 1;
    }
