// antsrl_memnet_body.inc — the bf16 forward of the memory agent's net behind a wave's place in the batch, ONE text
// included inside k_memnet (antsrl_memnet.hip) and k_pop_memnet (antsrl_popmemnet.hip); see antsrl_policy_flat_body.inc
// for why it is an include (and antsrl_memnet_dev.h: as a shared function it changes k_memnet's schedule).  Reads the
// including kernel's `pk` (the pack), `io`, `d`, `L`, `wcap`, its template flag OBS16 and what the kernel's prologue
// made of them: lane, r, h, Dp, stride, xt (the wave's LDS tile), wbuf (the shared weight chunk), t0 (the wave's first
// ant), ant (this lane's, clamped to io.M - 1) and live (this lane writes).  Everything it reads or writes of the batch
// goes through io and `ant` / t0 below io.M: a kernel that has moved io to a member's rows stays inside them.

    // ---- stage x (bf16) in the wave's LDS tile: 32-column chunks, lanes 0-31 on ant 2p and lanes 32-63 on ant 2p + 1
    // (128 coalesced bytes of a float32 row per half-wave), the 16 ant pairs' loads in flight together
    for (int c = 0; c < Dp / 32; ++c) {
        const int k = 32 * c + r;
        float xv[16];
        if (32 * c + 32 <= d.F) { // observation columns only
#pragma unroll
            for (int p = 0; p < 16; ++p) xv[p] = mn_obs<OBS16>(io, d, (size_t)min(t0 + 2 * p + h, io.M - 1), k);
        } else {                  // end of the row, agent_state, old memory, zero pad
#pragma unroll
            for (int p = 0; p < 16; ++p) xv[p] = mn_x<OBS16>(io, d, (size_t)min(t0 + 2 * p + h, io.M - 1), k);
        }
#pragma unroll
        for (int p = 0; p < 16; ++p) xt[(2 * p + h) * stride + k] = (__bf16)xv[p];
    }
    mn_tile_sync();
    const __bf16 *brow = xt + r * stride + 8 * h;

    bf16x8 u[2 * MN_MAXT], v[2 * MN_MAXT];
    // ---- trunk
    mn_layer_lds(pk, L, 0, brow, u, true, lane, h, wbuf, wcap); // L1
    mn_layer_reg(pk, L, 1, u, v, true, lane, h, wbuf, wcap);    // L2
    mn_layer_reg(pk, L, 2, v, u, true, lane, h, wbuf, wcap);    // L3
    mn_tile_sync(); // every lane's L1 reads of x are done before g overwrites it
    {
        // L4 + residual, one output tile at a time, into the LDS tile as g (bf16)
        const float *b = reinterpret_cast<const float *>(pk + L.bias_off[3]);
        for (int t = 0; t < L.tout[3]; ++t) {
            f32x16 acc = mn_tile_reg(mn_stage(pk, L, 3, t, wbuf, wcap), L.ks[3], u, lane);
            float bv[16], xr[16];
            mn_bias(b, t, h, bv);
            if (32 * t + 32 <= d.F) {
#pragma unroll
                for (int g = 0; g < 16; ++g) xr[g] = mn_obs<OBS16>(io, d, ant, 32 * t + (g & 3) + 8 * (g >> 2) + 4 * h);
            } else {
#pragma unroll
                for (int g = 0; g < 16; ++g) xr[g] = mn_x<OBS16>(io, d, ant, 32 * t + (g & 3) + 8 * (g >> 2) + 4 * h);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
                bf16x4 gv;
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[e] = (__bf16)((acc[4 * q + e] + bv[4 * q + e]) + xr[4 * q + e]);
                *reinterpret_cast<bf16x4 *>(xt + r * stride + 32 * t + 8 * q + 4 * h) = gv;
            }
        }
    }
    mn_tile_sync();

    // ---- rotation head: R3(R2(R1(g)))
    {
        mn_layer_lds(pk, L, 4, brow, u, false, lane, h, wbuf, wcap);
        mn_layer_reg(pk, L, 5, u, v, false, lane, h, wbuf, wcap);
        f32x16 q = mn_tile_reg(mn_stage(pk, L, 6, 0, wbuf, wcap), L.ks[6], v, lane);
        float bv[16];
        mn_bias(reinterpret_cast<const float *>(pk + L.bias_off[6]), 0, h, bv);
#pragma unroll
        for (int g = 0; g < 16; ++g) q[g] += bv[g];
        const int ar = mn_argmax(q, d.n_rot, h);
        if (live) {
            if (h == 0) io.rot[ant] = (int8_t)(ar - d.n_rot / 2);
            if (io.q_out) {
                const int nq = d.n_rot + d.n_ph;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                    if (row < d.n_rot) io.q_out[ant * nq + row] = q[g];
                }
            }
        }
    }
    // ---- pheromone head: P2(P1(g))
    {
        mn_layer_lds(pk, L, 7, brow, u, false, lane, h, wbuf, wcap);
        f32x16 q = mn_tile_reg(mn_stage(pk, L, 8, 0, wbuf, wcap), L.ks[8], u, lane);
        float bv[16];
        mn_bias(reinterpret_cast<const float *>(pk + L.bias_off[8]), 0, h, bv);
#pragma unroll
        for (int g = 0; g < 16; ++g) q[g] += bv[g];
        const int ap = mn_argmax(q, d.n_ph, h);
        if (live) {
            if (h == 0 && io.ph) io.ph[ant] = (int8_t)ap;
            if (io.q_out) {
                const int nq = d.n_rot + d.n_ph;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                    if (row < d.n_ph) io.q_out[ant * nq + d.n_rot + row] = q[g];
                }
            }
        }
    }
    // ---- memory: m = M2(M1(g)); new = tanh(M3 m) * s + old * (1 - s), s = sigmoid(Fg m)
    {
        mn_layer_lds(pk, L, 9, brow, u, false, lane, h, wbuf, wcap);
        mn_layer_reg(pk, L, 10, u, v, false, lane, h, wbuf, wcap);
        const float *b = reinterpret_cast<const float *>(pk + L.bias_off[11]);
        // both tiles in one staged chunk (2 x ks[11] <= 32 fragments): tile 1 follows tile 0
        const bf16x8 *A = mn_stage(pk, L, 11, 0, wbuf, wcap);
        f32x16 m3 = mn_tile_reg(A, L.ks[11], v, lane), fg = mn_tile_reg(A + L.ks[11] * 64, L.ks[11], v, lane);
        float b3[16], bf[16], old[16];
        mn_bias(b, 0, h, b3);
        mn_bias(b, 1, h, bf);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            old[g] = io.mem_in[ant * d.mem + min(row, d.mem - 1)]; // every read of this ant's row precedes the write
        }
        if (live)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                const float s = 1.0f / (1.0f + expf(-(fg[g] + bf[g])));
                const float nm = tanhf(m3[g] + b3[g]) * s + old[g] * (1.0f - s);
                if (row < d.mem) io.mem_out[ant * d.mem + row] = nm;
            }
    }
