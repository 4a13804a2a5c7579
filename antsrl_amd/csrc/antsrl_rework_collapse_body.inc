// antsrl_rework_collapse_body.inc — the body of k_rework_collapse (antsrl_rework.hip) and of k_pop_rework_collapse
// (antsrl_poprework.hip): one workgroup (blockIdx.x) per output row o of Wc.  The including kernel names `P` (P.p[t]:
// tensor t of the net, the state_dict's order), `d` (ReworkDims) and `collapsed` (float [NQ D + NQ], read and written one
// float at a time: 4-byte aligned and no more).
    __shared__ double vbuf[2][RW_MAX_D];
    const int o = blockIdx.x, tid = threadIdx.x;
    const bool rot = o < d.n_rot;
    const int start = rot ? 7 : 9, row = rot ? o : o - d.n_rot;
    const int npush = rot ? 7 : 5; // rotation_layer3, 2, 1, layer4, 3, 2, 1  /  pheromone_layer1, layer4, 3, 2, 1
    int width = rw_in(d, start);
    double *cur = vbuf[0], *nxt = vbuf[1];
    for (int c = tid; c < width; c += RW_TPB) cur[c] = (double)P.p[2 * start][(size_t)row * width + c];
    double bc = (double)P.p[2 * start + 1][row]; // (the last thread's is the one that counts)
    __syncthreads();
    for (int s = 0; s < npush; ++s) {
        const int l = rot ? 6 - s : (s == 0 ? 8 : 4 - s);
        const float *__restrict__ W = P.p[2 * l], *__restrict__ b = P.p[2 * l + 1];
        const int in = rw_in(d, l); // rw_out(d, l) == width
        for (int c = tid; c < in; c += RW_TPB) {
            double a = 0.0;
            for (int i = 0; i < width; ++i) a = a + cur[i] * (double)W[(size_t)i * in + c];
            nxt[c] = a;
        }
        if (tid == RW_TPB - 1)
            for (int i = 0; i < width; ++i) bc = bc + cur[i] * (double)b[i];
        __syncthreads();
        double *t = cur;
        cur = nxt;
        nxt = t;
        width = in;
    }
    // width == D
    const int NQ = d.n_rot + d.n_ph;
    for (int c = tid; c < d.D; c += RW_TPB) collapsed[(size_t)o * d.D + c] = (float)cur[c];
    if (tid == RW_TPB - 1) collapsed[(size_t)NQ * d.D + o] = (float)bc;
