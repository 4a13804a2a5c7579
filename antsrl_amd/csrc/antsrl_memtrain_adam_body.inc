// antsrl_memtrain_adam_body.inc — the body of k_mt_adam (antsrl_memtrain.hip) and of k_pop_mt_adam
// (antsrl_popmemtrain.hip): Adam on one trained element, then its two places in the bf16 packs (update = 0: repack
// only).  Names it reads: T (MtLayers), params, m, v, pack and grads of this kernel's net, update, step_size, bc2_sqrt,
// w1, beta2, w2, eps.
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= T.trained) return;
    float p = params[e];
    if (update) {
        const float g = grads[e];
        float mm = m[e], vv = v[e];
        p = adam_element(p, g, mm, vv, step_size, bc2_sqrt, w1, beta2, w2, eps); // antsrl_adam.h
        m[e] = mm;
        v[e] = vv;
        params[e] = p;
    }
    const int l = mt_layer_of(T, e);
    const size_t k = e - T.poff[l];
    if (k < (size_t)T.out[l] * T.in[l]) {
        const int o = (int)(k / T.in[l]), i = (int)(k % T.in[l]);
        const __bf16 pb = (__bf16)p;
        pack[T.woff[l] + (size_t)o * T.Kp[l] + i] = pb;
        pack[T.wtoff[l] + (size_t)i * T.Np[l] + o] = pb;
    }
