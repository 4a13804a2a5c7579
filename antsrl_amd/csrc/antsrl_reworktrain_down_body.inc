// antsrl_reworktrain_down_body.inc — the body of k_reworktrain_down (antsrl_reworktrain.hip) and of
// k_pop_reworktrain_down (antsrl_poprework.hip): one workgroup (blockIdx.x) per row o.  The including kernel names `a`,
// the step's ReworkTrainArgs (a member's own, in a population).
    __shared__ double vbuf[2][RW_MAX_D];
    const ReworkDims &d = a.d;
    const ReworkTrainLayout &L = a.L;
    const int o = blockIdx.x, tid = threadIdx.x, NQ = d.n_rot + d.n_ph;
    const bool rot = o < d.n_rot;
    const int last = rot ? 7 : 9, row = rot ? o : o - d.n_rot;
    const int npush = rot ? 7 : 5; // rotation_layer3, 2, 1, layer4, 3, 2, 1  /  pheromone_layer1, layer4, 3, 2, 1
    const float *__restrict__ P = a.model;
    // this row of M in the layers above layer4: zeros in the other head's, the unit row in its own last
    for (int l = 4; l < RW_LAYERS; ++l) {
        if ((l < 8) == rot && l != last) continue;
        double *M = reinterpret_cast<double *>(a.work + L.M[l]) + (size_t)o * L.out[l];
        for (int c = tid; c < L.out[l]; c += RT_TPB) M[c] = (l == last && c == row) ? 1.0 : 0.0;
    }
    int width = L.in[last];
    double *cur = vbuf[0], *nxt = vbuf[1];
    for (int c = tid; c < width; c += RT_TPB) cur[c] = (double)P[L.off[2 * last] + (size_t)row * width + c];
    double bc = (double)P[L.off[2 * last + 1] + row]; // (the last thread's is the one that counts)
    __syncthreads();
    for (int s = 0; s < npush; ++s) {
        const int l = rot ? 6 - s : (s == 0 ? 8 : 4 - s);
        const float *__restrict__ W = P + L.off[2 * l], *__restrict__ b = P + L.off[2 * l + 1];
        const int in = L.in[l]; // L.out[l] == width
        double *M = reinterpret_cast<double *>(a.work + L.M[l]) + (size_t)o * width;
        for (int c = tid; c < width; c += RT_TPB) M[c] = cur[c];
        for (int c = tid; c < in; c += RT_TPB) {
            double v = 0.0;
            for (int i = 0; i < width; ++i) v = v + cur[i] * (double)W[(size_t)i * in + c];
            nxt[c] = v;
        }
        if (tid == RT_TPB - 1)
            for (int i = 0; i < width; ++i) bc = bc + cur[i] * (double)b[i];
        __syncthreads();
        double *t = cur;
        cur = nxt;
        nxt = t;
        width = in;
    }
    // width == D
    float *collapsed = reinterpret_cast<float *>(a.work + L.collapsed);
    for (int c = tid; c < d.D; c += RT_TPB) collapsed[(size_t)o * d.D + c] = (float)cur[c];
    if (tid == RT_TPB - 1) collapsed[(size_t)NQ * d.D + o] = (float)bc;
