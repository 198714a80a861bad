// beam_wave_session.hip -- the beam-search session instantiations of beam_wave_kernel (SES, beam_wave.hip): every shape
// of the one-shot launcher, f32 and 16-bit posteriors, both tie orders, with and without the tie instrument -- and no
// UNI / PROF / NB variants.  A translation unit of its own, so that the build compiles it next to beam_wave.hip.
#define FCD_BEAM_WAVE_KERNEL_ONLY 1
#include "beam_wave.hip"

namespace fcd {

namespace {

template <int N, int GW, int RPW, int S, bool PDQ>
hipError_t ses_tp(const WaveParams &p, hipStream_t stream) {
    const int64_t waves = (p.in.n_reads + RPW - 1) / RPW;
    const dim3 grid((unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
    const bool amb = p.ses.count_amb != 0;
    if (p.in.dtype != kF32) {
        if (amb)
            hipLaunchKernelGGL((beam_wave_kernel<N, GW, RPW, S, true, false, false, true, PDQ, false, true>), grid, block, 0, stream, p);
        else
            hipLaunchKernelGGL((beam_wave_kernel<N, GW, RPW, S, false, false, false, true, PDQ, false, true>), grid, block, 0, stream, p);
    } else if (amb) {
        hipLaunchKernelGGL((beam_wave_kernel<N, GW, RPW, S, true, false, false, false, PDQ, false, true>), grid, block, 0, stream, p);
    } else {
        hipLaunchKernelGGL((beam_wave_kernel<N, GW, RPW, S, false, false, false, false, PDQ, false, true>), grid, block, 0, stream, p);
    }
    return hipGetLastError();
}

template <int N, int GW, int RPW, int S = 0>
hipError_t ses_t(const WaveParams &p, hipStream_t stream) {
    constexpr bool CAN_TIE = ((64 / RPW) / GW) * N > 20;  // (as launch_t)
    if (CAN_TIE && p.a.tie_order == FCD_TIE_PDQ178) return ses_tp<N, GW, RPW, S, CAN_TIE>(p, stream);
    return ses_tp<N, GW, RPW, S, false>(p, stream);
}

}  // namespace

// the shape choice of launch_beam_wave
hipError_t launch_beam_wave_session(const BatchDesc &in, int64_t n_reads, const BeamArgs &a, const WaveArena &arena,
                                    const ResultDesc &out, const SessionDesc &ses, hipStream_t stream) {
    if (n_reads <= 0) return hipSuccess;
    WaveParams p{in, a, arena, out, 0, NBestDesc{}, ses};
    p.in.n_reads = n_reads;
    const bool two = a.beam_size <= 5 && in.N <= 5 && !a.force_one_read_per_wave;
    const bool wide = a.beam_size > 8;
    if (a.crf) {
        if (!beam_wave_supported(a.beam_size, in.N, 1, in.S)) return hipErrorInvalidValue;
        if (in.S == 4) {
            if (wide) return ses_t<5, 5, 1, 4>(p, stream);
            return two ? ses_t<5, 6, 2, 4>(p, stream) : ses_t<5, 8, 1, 4>(p, stream);
        }
        if (wide) return ses_t<5, 5, 1, kCrfGather>(p, stream);
        return two ? ses_t<5, 6, 2, kCrfGather>(p, stream) : ses_t<5, 8, 1, kCrfGather>(p, stream);
    }
    if (wide) {
        switch (in.N) {
            case 3: return ses_t<3, 5, 1>(p, stream);
            case 4: return ses_t<4, 5, 1>(p, stream);
            case 5: return ses_t<5, 5, 1>(p, stream);
        }
        return hipErrorInvalidValue;
    }
    if (two) {
        switch (in.N) {
            case 3: return ses_t<3, 6, 2>(p, stream);
            case 4: return ses_t<4, 6, 2>(p, stream);
            case 5: return ses_t<5, 6, 2>(p, stream);
        }
    }
    switch (in.N) {
        case 3: return ses_t<3, 8, 1>(p, stream);
        case 4: return ses_t<4, 8, 1>(p, stream);
        case 5: return ses_t<5, 8, 1>(p, stream);
        case 6: return ses_t<6, 8, 1>(p, stream);
        case 7: return ses_t<7, 8, 1>(p, stream);
    }
    return hipErrorInvalidValue;
}

// this translation unit's copy of the replay's std-form word (pdq178.h), on the current device
FCD_PDQ178_DEFINE_STD_FORM_SETTER(beam_wave_session_set_pdq178_std_form)

}  // namespace fcd
