// antsrl_memtrain_gemm_body.inc — the body of k_mt_gemm (antsrl_memtrain.hip) and of k_pop_mt_gemm
// (antsrl_popmemtrain.hip): one wave per 32 x 32 output tile of the launch's grouped problems.  Names it reads: G (the
// kernel's MtGemm, as the host filled it) and `at`, which hands out an operand of G as this kernel's net reads it
// (MtAsFilled, or a population's member).  The grid's x dimension counts the workgroups.
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = blockIdx.x * MT_WAVES + (threadIdx.x >> 6);
    int pi = -1;
#pragma unroll
    for (int i = 0; i < MT_MAXP; ++i)
        if (i < G.np && wave >= G.p[i].tile0 && wave < G.p[i].tile0 + G.p[i].tiles) pi = i;
    if (pi < 0) return;
    const MtProb &P = at(G.p[pi]);
    const int t = wave - P.tile0, ntn = P.N / 32;
    const int m0 = (t / ntn) * 32, n0 = (t % ntn) * 32;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    const MtX &X = at(G.x[P.xnet]);
    acc = mt_segment(acc, P.a, P.lda, &X, P.w, P.ldw, P.K, m0 + r, n0 + r, h);
    if (P.a2) acc = mt_segment(acc, P.a2, P.lda2, &X, P.w2, P.ldw2, P.K2, m0 + r, n0 + r, h);
    const int j = n0 + r;
    const float bj = (P.bias && j < P.nb) ? P.bias[j] : 0.0f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int i = m0 + 8 * (g >> 2) + 4 * h + (g & 3);
        float v = acc[g] + bj;
        if (P.resid) v = v + mt_x(X, i, j);
        if (P.relu) v = fmaxf(v, 0.0f);
        if (P.mask) v = P.mask[(size_t)i * P.ldm + j] > 0.0f ? v : 0.0f;
        P.c[(size_t)i * P.ldc + j] = v;
    }
