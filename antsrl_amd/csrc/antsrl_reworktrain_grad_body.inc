// antsrl_reworktrain_grad_body.inc — the body of k_reworktrain_grad (antsrl_reworktrain.hip) and of
// k_pop_reworktrain_grad (antsrl_poprework.hip): one thread per trained float i, workgroups along x.  The including
// kernel names `a`, the step's ReworkTrainArgs (a member's own, in a population).
    const ReworkTrainLayout &L = a.L;
    const size_t i = (size_t)blockIdx.x * RT_TPB + threadIdx.x;
    if (i >= L.off[2 * RW_LAYERS]) return;
    int t = 0;
    for (int u = 1; u < 2 * RW_LAYERS; ++u) t += i >= L.off[u] ? 1 : 0;
    const int l = t >> 1, in = L.in[l], out = L.out[l], D = a.d.D, NQ = a.d.n_rot + a.d.n_ph;
    const size_t local = i - L.off[t];
    const bool bias = t & 1;
    const int o = bias ? (int)local : (int)(local / in), c = bias ? 0 : (int)(local - (size_t)o * in);
    const double *__restrict__ M = reinterpret_cast<const double *>(a.work + L.M[l]);
    const float *__restrict__ G = reinterpret_cast<const float *>(a.work + L.G), *__restrict__ S = G + (size_t)NQ * D;
    const int src = L.src[l];
    const double *__restrict__ A = reinterpret_cast<const double *>(a.work + L.A[src < 0 ? 0 : src]);
    double v = 0.0;
    for (int k = L.k0[l]; k < L.k1[l]; ++k) {
        const double x = bias ? (double)S[k] : (src < 0 ? (double)G[(size_t)k * in + c] : A[(size_t)k * in + c]);
        v = v + M[(size_t)k * out + o] * x;
    }
    const float g = (float)v;
    if (a.grads) a.grads[i] = g;
    if (a.adam.on) adam_at(a.model, a.adam, i, g);
