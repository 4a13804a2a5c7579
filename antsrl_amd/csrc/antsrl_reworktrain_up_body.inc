// antsrl_reworktrain_up_body.inc — the body of k_reworktrain_up (antsrl_reworktrain.hip) and of k_pop_reworktrain_up
// (antsrl_poprework.hip): one workgroup (blockIdx.x) per pseudo-row k.  The including kernel names `a`, the step's
// ReworkTrainArgs (a member's own, in a population).  The loss is written by thread RT_TPB - 65 of workgroup 0.
    __shared__ double vbuf[2][RW_MAX_D];
    __shared__ double s_sh;
    __shared__ float tail[3][RT_MAX_PARTS];
    const ReworkDims &d = a.d;
    const ReworkTrainLayout &L = a.L;
    const int k = blockIdx.x, tid = threadIdx.x, NQ = d.n_rot + d.n_ph, D = d.D;
    const bool rot = k < d.n_rot;
    const float *__restrict__ part = reinterpret_cast<const float *>(a.work + L.partials);
    const size_t PS = L.part_stride;
    float *G = reinterpret_cast<float *>(a.work + L.G), *S = G + (size_t)NQ * D;
    double *cur = vbuf[0], *nxt = vbuf[1];
    // s[k] and the two loss sums: the partials' values through LDS (loaded side by side), then added in workgroup order
    if (tid < L.parts) {
        tail[0][tid] = part[tid * PS + (size_t)NQ * D + k];
        tail[1][tid] = part[tid * PS + (size_t)NQ * D + NQ];
        tail[2][tid] = part[tid * PS + (size_t)NQ * D + NQ + 1];
    }
    for (int c = tid; c < D; c += RT_TPB) {
        float gsum = 0.0f;
#pragma unroll 8
        for (int w = 0; w < L.parts; ++w) gsum = gsum + part[w * PS + (size_t)k * D + c];
        G[(size_t)k * D + c] = gsum;
        cur[c] = (double)gsum;
    }
    __syncthreads();
    if (tid == RT_TPB - 1) {
        float ssum = 0.0f;
        for (int w = 0; w < L.parts; ++w) ssum = ssum + tail[0][w];
        S[k] = ssum;
        s_sh = (double)ssum;
    }
    if (k == 0 && tid == RT_TPB - 65) { // (another wave)
        float lr = 0.0f, lp = 0.0f;
        for (int w = 0; w < L.parts; ++w) {
            lr = lr + tail[1][w];
            lp = lp + tail[2][w];
        }
        *a.loss = lr * a.loss_rot + lp * a.loss_ph;
    }
    // this row of A in the other head's layers: zeros
    for (int l = 4; l < 9; ++l) {
        if (l == 7 || (l < 8) == rot) continue;
        double *A = reinterpret_cast<double *>(a.work + L.A[l]) + (size_t)k * L.out[l];
        for (int j = tid; j < L.out[l]; j += RT_TPB) A[j] = 0.0;
    }
    __syncthreads();
    const double sk = s_sh;
    const float *__restrict__ P = a.model;
    const int nlayers = rot ? 7 : 5; // layer1..4, then rotation_layer1..3 / pheromone_layer1
    for (int s = 0; s < nlayers; ++s) {
        const int l = (!rot && s == 4) ? 8 : s;
        const float *__restrict__ W = P + L.off[2 * l], *__restrict__ b = P + L.off[2 * l + 1];
        const int in = L.in[l], out = L.out[l];
        double *A = reinterpret_cast<double *>(a.work + L.A[l]) + (size_t)k * out;
        for (int j = tid; j < out; j += RT_TPB) {
            const float *__restrict__ w = W + (size_t)j * in;
            double v = 0.0;
            for (int c = 0; c < in; ++c) v = v + cur[c] * (double)w[c];
            v = v + sk * (double)b[j];
            nxt[j] = v;
            A[j] = v;
        }
        __syncthreads();
        double *t = cur;
        cur = nxt;
        nxt = t;
    }
