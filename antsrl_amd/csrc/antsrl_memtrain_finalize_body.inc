// antsrl_memtrain_finalize_body.inc — the body of k_mt_finalize (antsrl_memtrain.hip) and of k_pop_mt_finalize
// (antsrl_popmemtrain.hip): the chunk partials summed in ascending order into the flat gradient; the thread behind the
// last element sums the loss partials.  Names it reads: T (MtLayers), part, part_chunk, nchunk, grads, lossp, nloss and
// loss of this kernel's net; it leaves `e`, the thread's element (e == T.trained: the thread that wrote *loss).
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < T.trained) {
        const int l = mt_layer_of(T, e);
        const size_t k = e - T.poff[l], nw = (size_t)T.out[l] * T.in[l];
        const size_t src = T.part[l] + (k < nw ? (k / T.in[l]) * T.Kp[l] + k % T.in[l] : (size_t)T.Np[l] * T.Kp[l] + (k - nw));
        float s = 0.0f;
        for (int c = 0; c < nchunk; ++c) s += part[(size_t)c * part_chunk + src];
        grads[e] = s;
    } else if (e == T.trained) {
        float s = 0.0f;
        for (int i = 0; i < nloss; ++i) s += lossp[i];
        *loss = s;
    }
