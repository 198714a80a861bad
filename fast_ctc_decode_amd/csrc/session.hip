// session.hip -- the root state of beam-search session slots (fcd_beam_session_create / _restart, include/fcd.h).
// One wavefront per listed slot writes the state block the SES instantiations of the beam kernels load
// (fcd_internal.h SessionDesc): the search's first beam, search.rs:170-175 (root, label_prob 0, gap_prob 1) or, CRF,
// :54-59 (state = argmax(init), label_prob = max(init), gap_prob = init[0]; the first maximum wins).  A NaN init row, or
// a state the table does not hold, fails the slot's first non-empty push, as the one-shot kernels fail a read of T > 0.
#include "device_utils.h"
#include "fcd_internal.h"

namespace fcd {

namespace {

struct RestartParams {
    SessionDesc ses;
    const int64_t *slots;
    const float *init;  // [n_slots][n_init] (CRF)
    int64_t n_init;
    int wave, beam_size, NL, crf, S;
};

__global__ __launch_bounds__(64) void session_restart_kernel(RestartParams p) {
    const int lane = threadIdx.x;
    int32_t *blk = p.ses.state + p.slots[blockIdx.x] * p.ses.block_words;
    float lp = 0.0f, gp = 1.0f;
    int st = 0;
    bool bad = false;
    if (p.crf) {
        const float *init = p.init + (int64_t)blockIdx.x * p.n_init;
        float m = init[0];
        bad = m != m;
        for (int64_t j = 1; j < p.n_init; ++j) {
            const float e = init[j];
            bad = bad || (e != e);
            if (e > m) {
                m = e;
                st = (int)j;
            }
        }
        lp = m;
        gp = init[0];
    }
    if (lane == 0) {
        blk[0] = 1;  // B
        blk[1] = 1;  // alive
        blk[2] = FCD_ST_OK;
        blk[3] = 0;
        blk[4] = 0;
        blk[5] = 0;  // t0
        blk[6] = (p.wave && p.crf && (bad || st >= p.S)) ? 1 : 0;  // wave: bad init pending / generic: node count
        blk[7] = 0;
    }
    int32_t *b = blk + kSesHeader;
    if (p.wave) {
        // every lane's node, lp, gp, tipf, depth, jump, child, state (beam_wave.hip)
        b[lane] = -1;
        b[64 + lane] = __float_as_int(lp);
        b[128 + lane] = __float_as_int(gp);
        b[192 + lane] = 0;
        b[256 + lane] = 0;
        b[320 + lane] = -1;
        b[384 + lane] = -1;
        b[448 + lane] = (bad || st >= p.S) ? 0 : st;
    } else {
        // beam buffer 0 of beam_generic.hip's Lds: node, lp, gp, tip, par, state, depth (BC each), child (BC * NL)
        const int BC = p.beam_size;
        if (lane == 0) {
            b[0] = -1;
            b[BC] = __float_as_int(lp);
            b[2 * BC] = __float_as_int(gp);
            b[3 * BC] = -1;
            b[4 * BC] = -2;
            b[5 * BC] = bad ? -1 : st;  // (out of range: the first step fails the slot)
            b[6 * BC] = 0;
        }
        for (int j = lane; j < p.NL; j += 64) b[7 * BC + j] = -1;
    }
}

}  // namespace

hipError_t launch_session_restart(const SessionDesc &ses, const int64_t *slots, int64_t n_slots, bool wave, int beam_size,
                                  int N, int crf, int S, const float *init, int64_t n_init, hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    RestartParams p{ses, slots, init, n_init, wave ? 1 : 0, beam_size, N - 1, crf, S};
    hipLaunchKernelGGL(session_restart_kernel, dim3((unsigned)n_slots), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace fcd
