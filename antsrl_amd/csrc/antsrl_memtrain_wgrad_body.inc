// antsrl_memtrain_wgrad_body.inc — the body of k_mt_wgrad (antsrl_memtrain.hip) and of k_pop_mt_wgrad
// (antsrl_popmemtrain.hip): one wave per (row chunk, 32 x 32 tile of dW).  Names it reads: G (the kernel's MtWgrad, as
// the host filled it) and `at`, which hands out an operand of G as this kernel's net reads it (at(G.p[i]), at(G.x),
// at.work(G.part)).
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = blockIdx.x * MT_WAVES + (threadIdx.x >> 6);
    int pi = -1;
    for (int i = 0; i < G.np; ++i)
        if (wave >= G.p[i].tile0 && wave < G.p[i].tile0 + G.p[i].tiles) pi = i;
    if (pi < 0) return;
    const MtWg &P = at(G.p[pi]);
    const MtX &X = at(G.x);
    const int tpc = (P.Np / 32) * (P.Kp / 32), t = wave - P.tile0;
    const int c = t / tpc, o0 = ((t % tpc) / (P.Kp / 32)) * 32, i0 = ((t % tpc) % (P.Kp / 32)) * 32;
    const int b0 = c * G.chunk, b1 = min(b0 + G.chunk, G.Bp);
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    for (int k0 = b0; k0 < b1; k0 += 16) {
        bf16x8 av, bv;
        const size_t kb = (size_t)(k0 + 8 * h);
#pragma unroll
        for (int j = 0; j < 8; ++j) av[j] = (__bf16)P.dy[(kb + j) * P.lddy + o0 + r];
        if (P.x) {
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[j] = (__bf16)P.x[(kb + j) * P.ldx + i0 + r];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[j] = (__bf16)mt_x(X, (int)kb + j, i0 + r);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
    }
    float *out = at.work(G.part) + (size_t)c * G.part_chunk + P.off;
#pragma unroll
    for (int g = 0; g < 16; ++g) out[(size_t)(o0 + 8 * (g >> 2) + 4 * h + (g & 3)) * P.Kp + i0 + r] = acc[g];
    if (i0 == 0 && h == 0) { // db over the chunk, fp32, rows in order
        float s = 0.0f;
        for (int b = b0; b < b1; ++b) s += P.dy[(size_t)b * P.lddy + o0 + r];
        out[(size_t)P.Np * P.Kp + o0 + r] = s;
    }
