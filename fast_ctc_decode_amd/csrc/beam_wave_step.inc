// beam_wave_step.inc -- one time step of beam_wave_kernel (beam_wave.hip): the body of its time loop.  Nothing the step
// reads is changed before its last block (the commit).  PDQ: a step whose kept candidates tie among more than 20 has
// its exact ranks replaced by the quicksort's (pdq178_wave.h) inside the step's one rare branch and everything that
// depends on the ranks run again.  (r04: a second copy of the step one loop level up, entered by leaving the time loop,
// cost 7 % -- a loop with two exits gets a guard variable and a dozen scalar instructions per step from LLVM's
// loop-exit unification, and the kernel is bound by the LATENCY of its dependent chain: every instruction and every
// wait on the path shows.)
        const bool act0 = UNI ? alive : (alive && t < T);
        const bool act = act0;
        const int tks = SES ? (t0 + t) << KS : t << KS;  // first node id of the step (SES: absolute time)
        float pk = GATHER ? rowv : pk_next;
        const float pr0 = pk;
        const float ptip = ptip_next;
        stamp_f(0, pk);  // loop overhead + posterior row
        // HL: the step's lane predicates are formed as MASKS -- a vote on each bare compare (one instruction, exec is all
        // ones on this path), joined in scalar registers with the lane-constant masks balloted in front of the time loop
        // (beam_wave.hip: child_m, self_m, collapse_m) -- and read back as lane flags with lane_in(), which costs nothing.
        // A vote on a flag DERIVED from several compares costs two vector instructions (a 0 / 1 word and its compare with 0):
        // that is what m_new, m_valid, the clash vote and the rank-domain guard were.
        // WSC: m_grp is not voted on: it is the carried mask (beam_wave.hip: grp_m), set behind the rank of the step that last
        // changed a half's width.  The step reads this copy to its end; grp_m itself may already belong to the next one.
        const uint64_t m_grp = HL ? (WSC ? grp_m : ballot(i < B)) : 0ull;
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: there the per-lane B is carried along with the scalar state)
        if (WSC && (m_grp != ballot(i < B) || B != (hbase ? width1 : width0))) {
            fprintf(stderr, "beam_wave: carried group mask %016llx / widths %d, %d, but lane %d holds beam width %d\n",
                    (unsigned long long)m_grp, width0, width1, lane, B);
            abort();
        }
#endif
        const uint64_t m_rep = HL ? (collapse_m & ballot((k << 2) == tipf)) : 0ull;
        const uint64_t m_ex = HL ? ballot(child >= 0) : 0ull;
        // (exists && IN-BEAM in one compare: the sign bit clear and the flag set)
        const uint64_t m_ib = HL ? ballot((child & (kInBeam | (int)0x80000000)) == kInBeam) : 0ull;
        const uint64_t m_cv = HL ? (m_grp & child_m & ballot(!(pk < thr)) & (m_ex | ~m_rep | ballot(gp > 0.0f))) : 0ull;
        const uint64_t m_mg = m_cv & m_ib;
        const bool grp = HL ? lane_in(m_grp, lane) : (UNI ? i < B : (act && i < B));

        // ---- child lanes: extension by label l (:200-239) ----
        const bool pass = !(pk < thr);  // :201 skips only when pr_b < thr
        const bool rep = HL ? lane_in(m_rep, lane) : (collapse && (k << 2) == tipf);  // l == tip
        const float contrib = rep ? gp * pk : (lp + gp) * pk;
        const bool exists = child >= 0;
        const int cid = child & kIdMask;
        const bool inbeam = HL ? lane_in(m_ib, lane) : (exists && (child & kInBeam));
        const int mslot = (child >> kSlotShift) & kSlotMask;
        const bool cvalid = HL ? lane_in(m_cv, lane)
                               : (grp && is_child && pass && (exists || !rep || gp > 0.0f));  // :212-218
        const bool merged = HL ? lane_in(m_mg, lane) : (cvalid && inbeam);  // the target's own lane 0 absorbs this extension
        // HL: the target slot's own lane as a byte address, formed once for the push here and the look-up behind the rank
        const int tgt_a = hbase_a + mslot * (GW << 2);
        const int dst = merged ? hbase + mslot * GW : dummy;
        const int dst_a = merged ? tgt_a : dummy_a;
        float inc = __int_as_float(HL ? __builtin_amdgcn_ds_permute(dst_a, __float_as_int(merged ? contrib : 0.0f))
                                      : perm(dst, __float_as_int(merged ? contrib : 0.0f)));
        const int incv = HL ? __builtin_amdgcn_ds_permute(dst_a, merged ? 1 : 0) : perm(dst, merged ? 1 : 0);
        stamp_f(1, inc);  // extensions + the push into slots that are beam entries

        // ---- self lanes: blank (:191-198) + repeat-stay (:206-211) + incoming extension ----
        const uint64_t m_blank = HL ? ballot(pr0 > thr) : 0ull;
        const uint64_t m_stay = HL ? (collapse_m & ballot(tipf != 0) & ballot(!(ptip < thr))) : 0ull;
        const uint64_t m_inc = HL ? (self_m & ballot(incv != 0)) : 0ull;
        // HL: the mask of this step's candidates.  It IS the vote "key != 0" (m_valid) the other instantiations take behind
        // the rank: their key is formed under exactly this mask and make_key() is never 0.  (RAWK: the table word below is
        // written under it and may well be 0 for a candidate -- p = 0 -- so nothing reads validity off a word.)
        const uint64_t m_val = HL ? ((m_grp & self_m & (m_blank | m_stay | m_inc)) | (m_cv & ~m_ib)) : 0ull;
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu)
        // what the eviction mask below rests on: a candidate lane that is no child lane is a slot's own lane
        if (HL && (m_val & ~child_m) != (m_val & self_m)) {
            fprintf(stderr, "beam_wave: a candidate on a lane that is neither a slot's own nor a child lane\n");
            abort();
        }
#endif
        const bool blank = HL ? lane_in(m_blank, lane) : (pr0 > thr);
        const float gpn = (lp + gp) * pr0;
        const bool stay = HL ? lane_in(m_stay, lane) : (collapse && tipf != 0 && !(ptip < thr));
        const float lpn = lp * ptip;
        const bool has_inc = HL ? lane_in(m_inc, lane) : (is_self && incv != 0);
        // ZSEL: `inc` as it arrived.  Only a slot's own lane reads slp (clp, below), and a slot's own lane is the push target of
        // merged extensions alone -- every other lane pushes to its group's spare lane or, an idle lane, to itself (dummy_a) --
        // so one that nobody pushed to is a lane no ds_permute source addresses, and such a lane receives 0: bit pattern 0, the
        // +0.0f the select put there.  (tests/hipemu's ds_permute does the same.)
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu)
        if (ZSEL && is_self && incv == 0 && __float_as_int(inc) != 0) {
            fprintf(stderr, "beam_wave: lane %d received no extension but holds the word %08x\n", lane, (unsigned)__float_as_int(inc));
            abort();
        }
#endif
        const float slp = (stay ? lpn : 0.0f) + (ZSEL ? inc : (has_inc ? inc : 0.0f));
        // ZSEL: sgp under "a slot's own or a group's spare lane, and the blank passes" -- zero on child and idle lanes by the mask,
        // so it IS cgp on every lane, and the spare lane's arm of dv (below) as before.  (A spare lane's prob is then
        // contrib + sgp instead of contrib: no lane but a candidate's has its prob read, and a spare lane holds none.)
        const float sgp = (ZSEL ? lane_in(gap_m & m_blank, lane) : blank) ? gpn : 0.0f;
        const bool svalid = grp && is_self && (blank || stay || has_inc);

        // (svalid / cvalid already carry is_self / is_child)
        const bool valid = HL ? lane_in(m_val, lane) : (svalid || (cvalid && !merged));
        const float clp = is_self ? slp : contrib;
        const float cgp = ZSEL ? sgp : (is_self ? sgp : 0.0f);
        const float prob = clp + cgp;

        const uint64_t m_isnew = m_cv & ~m_ex;  // (HL)
        const bool is_new = HL ? lane_in(m_isnew, lane) : (cvalid && !exists);

        // ---- prune, first half: sort keys out, comparands back (exact rank on (probability desc, node asc)) ----
        // The key needs a node index only to break probability ties, and only its ORDER matters: a node
        // created in this step gets (t << KS) + q here -- above every existing index and increasing with the
        // lane, exactly like the index it is about to receive -- so the key does not wait for the numbering below.
        // (A NaN key is garbage but non-zero: it only ever ranks when it is the read's lone candidate, :262.  Its
        // probability word may be 0 -- the negative NaN with an all-ones payload -- so "is a candidate" stays key != 0.)
        // (RAWK: idk is not formed.  The rare block takes the node word from `id`, where a new node carries the index the
        // numbering gave it: the same order as (t << KS) + q, by the argument above -- stated again where it is formed.)
        const int idk = is_self ? node : (is_new ? tks + q : cid);
        // kRawTop (HL): what the candidate leaves next to its survivor-table entry is its probability as make_key() takes it,
        // prob + 0.0f -- formed once, in front of the key's exec region, for both (formed again from the key where a tie replay
        // has parked the step's registers)
        float pcanon = prob + 0.0f;
        if (kRawTop) FCD_OPAQUE_VQ(pcanon);
        int pword = kRawTop ? __float_as_int(pcanon) : 0;
        // RAWK: no key here at all.  The every-step path ranks on the RAW probability word (below) and reads neither the
        // keyed word nor the node word; the step's rare block forms both, for every lane, when it is entered for a recount.
        uint64_t key = RAWK ? 0ull
                            : ((UNI ? valid : (valid && act)) ? (kRawTop ? make_key_canonical(pcanon, idk) : make_key(prob, idk)) : 0ull);
        // R32: the probability word and the node word go to two tables (beam_wave.hip), one ds_write2_b32; the rank below
        // is taken on the probability word alone, and candidates of equal probability are told apart only in the step's
        // rare branch, when the survivor table shows that two KEPT ones met (settle_table).
        // RAWK: ONE table word per step, the candidate's probability itself -- bits(pcanon), 0 on a lane without a candidate
        // (device_utils.h, FCD_RANKP4: what the count, the guard, an empty slot and a candidate of probability 0 make of it).
        // pcanon, not prob: the survivor table's tie words compare bit patterns, and -0.0 must not appear there.
        const uint32_t kp = RAWK ? (valid ? (uint32_t)pword : 0u) : (uint32_t)(key >> 32);
        if (RAWK) {
            kwords[kslot] = kp;
        } else if (R32) {
            kwords[kslot] = kp;
            kwords[kslot + kNodeTab] = (uint32_t)key;
        } else {
            keys[lane] = key;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        constexpr int NC = BCAP * N;  // comparand u = (slot u / N, column u % N)
        uint64_t kk[NC];
        // STREAM: the comparands are not all fetched up front (2 * NC registers, the largest live set of the step and what
        // held the kernel at four wavefronts per SIMD) but in blocks of four, kAhead blocks before the block that counts
        // them.  A slot's keys are contiguous and start on 16 bytes, so its columns leave two per ds_read_b128 -- the
        // paired columns of all slots first, an odd last column of every slot (one ds_read_b64 each) after them; the order
        // in which larger keys are counted is immaterial.
        constexpr int NPR = (N / 2) * 2;   // columns of a slot that travel in pairs
        constexpr int NP = BCAP * NPR;     // comparands v < NP: (slot v / NPR, column v % NPR); v >= NP: (slot v - NP, column N - 1)
        constexpr int NBLK = (NC + 3) / 4;
        constexpr int kAhead = 2;
        // R32: the half's probability words are contiguous -- block j is words 4j .. 4j + 3, one ds_read_b128 (the last block
        // what is left: one word when N = 5)
        uint32_t kw[NC];
        auto load_blk = [&](int j) __attribute__((always_inline)) {
            if (R32) {
                if (4 * j + 4 <= NC) {
                    uint32_t four[4];
                    __builtin_memcpy(four, __builtin_assume_aligned(&kwords[hw + 4 * j], 16), 16);
#pragma unroll
                    for (int v = 0; v < 4; ++v) kw[4 * j + v] = four[v];
                } else {
#pragma unroll
                    for (int v = 4 * j; v < NC; ++v) kw[v] = kwords[hw + v];
                }
                return;
            }
#pragma unroll
            for (int v = 4 * j; v < 4 * j + 4 && v < NC; ++v) {
                if (v < NP) {
                    if ((v & 1) == 0) {
                        uint64_t two[2];
                        __builtin_memcpy(two, __builtin_assume_aligned(&keys[hbase + (v / NPR) * GW + (v % NPR)], 16), 16);
                        kk[v] = two[0];
                        kk[v + 1] = two[1];
                    }
                } else {
                    kk[v] = keys[hbase + (v - NP) * GW + (N - 1)];
                }
            }
        };
        if (STREAM) {
#pragma unroll
            for (int j = 0; j < kAhead && j < NBLK; ++j) load_blk(j);
        } else {
#pragma unroll
            for (int u = 0; u < NC; ++u) kk[u] = keys[hbase + (u / N) * GW + (u % N)];
        }

        // ---- tree.rs:125-145 add_node: ids in (beam order, label order) == lane order; runs under the LDS reads ----
        const uint64_t m_new = HL ? m_isnew : ballot(is_new);
        const uint32_t w_new = RPW == 1 ? 0u : (hbase ? (uint32_t)(m_new >> 32) : (uint32_t)m_new);
        int pre_new;
        if (RPW == 1) {
            pre_new = popc64(m_new & lanemask_lt());
        } else if (HL) {
            pre_new = 0;  // (counted onto tks below)
        } else {
            pre_new = __builtin_popcount(w_new & ((1u << q) - 1u));
        }
        // < cap: the host sizes every slab for (T << KS) ids (capi.hip)
        const int newid = HL ? half_prefix_count(m_new, lane, low_half_v, tks) : tks + pre_new;
        // (beam_lane.hip writes a node's record when it first ENTERS THE BEAM -- a sixth of the stores.  Tried here, r05:
        // the stores ride for free under the LDS reads above, while next to the survivor gather they cost the PDQ
        // instantiation 8 B of scratch and 1 % -- the write traffic is not what bounds this kernel.)
        if (HL) {
            // one exec region for the record store; the segment-head store (one depth in 64) waits behind a wave-uniform
            // vote instead of a second region inside the first
            if (is_new) *at32(rec_w, hoff + (uint32_t)newid) = ((node + 1) << 3) | l;
            static_assert(kSeg == 64, "(depth + 1) % kSeg == 0 as a compare of the low six bits");
            const uint64_t m_head = m_new & ballot((depth & ((kSeg - 1) << kDsh)) == ((kSeg - 1) << kDsh));
            if (__builtin_expect(m_head != 0ull, 0)) {
                if (lane_in(m_head, lane)) *at32(jmp_w, hoff + (uint32_t)newid) = ((depth >> kDsh) % kSeg == 0) ? node : jump;
            }
        } else if (is_new) {
            *at32(rec_w, hoff + (uint32_t)newid) = ((node + 1) << 3) | l;
            // a segment head (depth % 64 == 0) records where the next head up the tree is
            if ((depth + 1) % kSeg == 0) *at32(jmp_w, hoff + (uint32_t)newid) = (depth % kSeg == 0) ? node : jump;
        }
        int child_in = is_new ? newid : child;  // (the entry as the rest of the step sees it)
        // (HL: a child lane's id is the id field of its entry as the step sees it -- a new id fits the field -- one select fewer)
        int id = is_self ? node : (HL ? (child_in & kIdMask) : (is_new ? newid : cid));
        stamp_i(2, id);  // own candidate, key, node numbering, record stores

        // ---- prune, second half: count the larger keys ----
        int rank = 0;
        const float fown_g = RAWK ? fcd_rankp_own(kp) : 0.0f;  // (HL: the count's own term; the guard votes on it as well)
        int n_eq = 0, n_gt = 0;  // AMB: candidates of exactly this probability (itself included) / of a greater one
        if (AMB) {
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                rank += (kk[u] > key) ? 1 : 0;
                n_eq += (kk[u] != 0ull && (uint32_t)(kk[u] >> 32) == (uint32_t)(key >> 32)) ? 1 : 0;
                n_gt += ((uint32_t)(kk[u] >> 32) > (uint32_t)(key >> 32)) ? 1 : 0;
            }
        } else if (STREAM) {
            // four independent compare-and-count chains (device_utils.h); the scheduling barriers keep the loads of block
            // j + kAhead behind the count of block j - 1 (left alone, the scheduler hoists every load to the top again)
            int r0, r1 = 0, r2 = 0, r3 = 0;
            static_assert(!STREAM || NC >= 4, "at least one block of four comparands");
            // HL: the count as a sum of clamped f32 differences (device_utils.h, FCD_RANKP4): own word scaled once
            const float fown = fown_g;
            float facc;
#pragma unroll
            for (int j = 0; j < NBLK; ++j) {
                __builtin_amdgcn_sched_barrier(0);
                if (j + kAhead < NBLK) load_blk(j + kAhead);
                if (R32 && HL) {  // the same count in ONE accumulator, in f32: v_fma_f32 + v_add_f32 per comparand
                    if (j == 0) {
                        FCD_RANKP4_FIRST(fown, kw[0], kw[1], kw[2], kw[3], facc);
                    } else if (4 * j + 4 <= NC) {
                        FCD_RANKP4(fown, kw[4 * j], kw[4 * j + 1], kw[4 * j + 2], kw[4 * j + 3], facc);
                    } else {
#pragma unroll
                        for (int u = 4 * j; u < NC; ++u) FCD_RANKP1(fown, kw[u], facc);
                    }
                } else if (R32) {  // r32 = #(probability word > own): candidates of equal probability share it
                    if (j == 0) {
                        FCD_RANK4_32_FIRST(kp, kw[0], kw[1], kw[2], kw[3], r0, r1, r2, r3);
                    } else if (4 * j + 4 <= NC) {
                        FCD_RANK4_32(kp, kw[4 * j], kw[4 * j + 1], kw[4 * j + 2], kw[4 * j + 3], r0, r1, r2, r3);
                    } else {
#pragma unroll
                        for (int u = 4 * j; u < NC; ++u) r0 += (kw[u] > kp) ? 1 : 0;
                    }
                } else if (j == 0) {
                    FCD_RANK4_FIRST(key, kk[0], kk[1], kk[2], kk[3], r0, r1, r2, r3);
                } else if (4 * j + 4 <= NC) {
                    FCD_RANK4(key, kk[4 * j], kk[4 * j + 1], kk[4 * j + 2], kk[4 * j + 3], r0, r1, r2, r3);
                } else {
#pragma unroll
                    for (int u = 4 * j; u < NC; ++u) r0 += (kk[u] > key) ? 1 : 0;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            rank = (R32 && HL) ? (int)facc : (r0 + r1) + (r2 + r3);  // (facc: a sum of 25 values in [0, 1])
        } else {
            // four independent compare-and-count chains (device_utils.h)
            int r0, r1, r2, r3;
            static_assert(NC >= 4, "at least one block of four comparands");
            FCD_RANK4_FIRST(key, kk[0], kk[1], kk[2], kk[3], r0, r1, r2, r3);
#pragma unroll
            for (int u = 4; u + 4 <= NC; u += 4) FCD_RANK4(key, kk[u], kk[u + 1], kk[u + 2], kk[u + 3], r0, r1, r2, r3);
#pragma unroll
            for (int u = NC & ~3; u < NC; ++u) r0 += (kk[u] > key) ? 1 : 0;
            rank = (r0 + r1) + (r2 + r3);
        }
        __builtin_amdgcn_wave_barrier();
        stamp_i(3, rank);  // exact rank

        // ---- search.rs:261-277 ----
        // (key != 0 <=> valid && act: a vote on a compare costs one instruction, a vote on a derived flag two)
        const uint64_t m_valid = HL ? m_val : ballot(key != 0ull);
        // (WSC: read only inside the rare blocks, where the compiler forms it)
        int n_valid = RPW == 1 ? popc64(m_valid)
                               : __builtin_popcount(hbase ? (uint32_t)(m_valid >> 32) : (uint32_t)m_valid);
        // WSC: what the every-step path keeps of the width -- the two halves' candidate counts, capped, against the carried
        // widths: four scalar counts and minima, two scalar differences.  A half whose width changes has a non-zero word.
        const int cap0 = WSC ? min(__builtin_popcount((uint32_t)m_valid), beam_size) : 0;
        const int cap1 = WSC ? min(__builtin_popcount((uint32_t)(m_valid >> 32)), beam_size) : 0;
        // (WSC: the one later reader of m_grp, the eviction mask, takes its part here, so that the carried mask is dead when the
        // block below forms the next step's and the two need not live side by side)
        const uint64_t m_cgrp = WSC ? (child_m & m_grp) : 0ull;
        const uint64_t m_width = WSC ? (((uint64_t)(uint32_t)(cap1 ^ width1) << 32) | (uint32_t)(cap0 ^ width0)) : 0ull;
        // Everything that ends a read is rare: one wave-wide test, the bookkeeping behind it.
        const bool is_nan = valid && prob != prob;
        // HL: a candidate whose probability word is outside the range on which the f32 count is exact (device_utils.h,
        // fcd_rankf_outside_m: three votes on bare compares of prob and of fown, which the count already holds).  It
        // sends the step to the exact recount (m_clash, below).
        const uint64_t m_guard = (R32 && HL) ? (fcd_rankf_outside_m(prob, fown_g, rankf_lo, rankf_hi) & m_valid) : 0ull;
        // HL: the same test on masks -- a half runs when alive_m says so.  A NaN's word is outside the rank domain whatever
        // its sign and payload (fcd_rankf_outside_m), so the guard's vote stands in for "some candidate is a NaN" here and the
        // every-step path takes no vote on prob != prob: a guarded step without a NaN enters the block and leaves it unchanged.
        // (HL: marked unlikely, so that the block sits behind the loop and the every-step path falls through)
        // WSC: "some running half's width changes" takes the place of the vote on n_valid == 0 -- an empty half's capped count
        // is 0, and a running half's width is at least 1 (it starts at 1, and a half left with none stops running in that
        // very step).  A half that does not run never changes: its group mask is empty, so it has no candidates and width 0.
        if (HL ? __builtin_expect((((WSC ? m_width : ballot(n_valid == 0)) | m_guard) & alive_m) != 0ull, 0)
               : (ballot(act && (n_valid == 0 || is_nan)) != 0ull)) {
            const bool act = HL ? lane_in(alive_m, lane) : act0;
            if (WSC) {
                // the per-lane count, formed HERE from a word the optimiser cannot see through: shared with the count behind
                // the block, it is computed in front of the branch, in every step
                uint32_t half_w = hbase ? (uint32_t)(m_valid >> 32) : (uint32_t)m_valid;
                FCD_OPAQUE_V(half_w);
                n_valid = __builtin_popcount(half_w);
            }
            const uint64_t m_nan = ballot(is_nan);
            const bool any_nan = RPW == 1 ? m_nan != 0ull
                                          : (hbase ? (uint32_t)(m_nan >> 32) : (uint32_t)m_nan) != 0u;
            const bool f_nan = act && n_valid >= 2 && any_nan;  // a lone NaN is never compared (:262)
            const bool f_empty = act && n_valid == 0;
            if (f_nan || f_empty) {
                if (SES) {
                    ses_st = f_empty ? FCD_ST_RAN_OUT_OF_BEAM : FCD_ST_INCOMPARABLE;
                } else if (q == 0) {
                    const int64_t rr = read_index_again();
                    p.out.status[rr] = f_empty ? FCD_ST_RAN_OUT_OF_BEAM : FCD_ST_INCOMPARABLE;
                    if (!NB) p.out.out_len[rr] = 0;  // (n-best rows: the epilogue)
                }
                if (!HL) alive = false;  // (HL: alive_m, below)
                if (UNI) n_valid = 0;  // the failed read keeps an empty beam from here on
            }
            if (HL) alive_m &= ~ballot(f_nan || f_empty);
            if (WSC) {
                // the next step's width, per half, from the per-lane count (0 by now for a half that has just failed); a
                // half whose width stays is written over with what it holds
                const int bn = n_valid < beam_size ? n_valid : beam_size;
                grp_m = ballot(i < bn);
                width0 = __builtin_amdgcn_readlane(bn, 0);
                width1 = __builtin_amdgcn_readlane(bn, HALF & 63);
            }
        }
        const bool go = UNI ? true : (act && alive);  // this half completes the step

        // WSC: the count and the width the later rare blocks read (the returning-node reload, the recount, the replay) are
        // functions of masks and scalar state the step holds anyway, and are formed where those blocks are entered (below)
        const int Bn = WSC ? (hbase ? width1 : width0) : (n_valid < beam_size ? n_valid : beam_size);
        // ---- keep the IN-BEAM/slot bits of every child entry current ----
        // an entry whose node is a beam entry follows that entry's own candidate: where did it go?
        // selflag = rank | 16 for a kept candidate, 0 otherwise: shifted to kSlotShift it IS the (slot, IN-BEAM)
        // field of a child entry (kInBeam == 16 << kSlotShift), so following an entry needs no compare
        static_assert(kInBeam == (16 << kSlotShift) && kSlotMask == 15, "child-entry bit layout");
        // Survivor table: entry r = the lane whose candidate took rank r.  LDS executes a wavefront's operations
        // in order, so the store, the read-back and the look-ups below (HL: one, `fate`) share ONE round trip (a ds_permute
        // to the new slot followed by a broadcast to its group were two dependent ones).
        const int depc = depth + (is_child ? (1 << kDsh) : 0);  // (HL: depth and depc are shifted up by kDsh = 8)
        bool sel;
        int selflag, fate, own, src_a, e_min, top_a, gp_a;
        int child_s;  // the entry after this step's bookkeeping
        int n_node, n_meta, n_state, n_jump, n_child;
#ifdef FCD_HIPEMU
        int n_child_kind = -1;
#endif
        float n_lp, n_gp, top;
        float dv = 0.0f;  // DSRC: what this lane divides by the top probability (not const: PARK)
        uint32_t tie0 = 0, tie1 = 1;
        bool clash = false;  // R32: this lane's entry of the survivor table was overwritten by a candidate of equal probability
        uint64_t m_sel = 0ull, m_clash_t = 0ull;  // HL: `sel` and `clash` as masks
        // Everything that depends on the ranks: survivor table, fate of the child entries, row eviction, the gather of
        // the survivors into rank order.  PDQ: it runs on the exact ranks first; the tie table comes back with the
        // same LDS round trip and is looked at only when the gather has landed -- a flagged step (rare) replaces the
        // ranks and settles again.  (An eviction store of the first pass that the second does not repeat leaves a row
        // in HBM nobody reads before it is written again: rows are read back only after their node's LAST eviction.)
        auto settle_table = [&]() __attribute__((always_inline)) {
            int m_chw = 0;  // (CHB: bit 0 of this lane's source entry, spread over the word)
            sel = valid && go && rank < beam_size;
            if (HL) {  // (a statement of its own: folded into the line above it changed the code of every other instantiation)
                m_sel = m_val & ballot(rank < beam_size);
                sel = lane_in(m_sel, lane);
            }
            selflag = sel ? (rank | 16) : 0;
            // PDQ: EVERY candidate leaves its entry (the table has room for all ranks; entries past the new beam are
            // never used as sources, and as depths they are not looked at), and next to it, kTie words further on, its
            // probability (orderable bits): rank i ties with rank i + 1 when the two words are equal.  One
            // ds_write2_b32 under the mask the step already holds -- no test of the rank at all.
            // DSRC: the exact-rank instantiations leave the probability word next to the entry as well (the same
            // ds_write2_b32) -- rank 0's is the step's divisor, and it comes back with the table's own round trip.
            const int ent = ent_lo | (HL ? depc : depc << 8);
            if (PDQ) {
                if (valid && go) {
                    srcs[rank] = ent;
                    srcs[kTie + rank] = kRawTop ? pword : (int)(uint32_t)(key >> 32);
                }
            } else if (DSRC) {
                if (sel) {
                    srcs[rank] = ent;
                    srcs[kTop + rank] = kRawTop ? pword : (int)(uint32_t)(key >> 32);
                }
            } else {
                if (sel) srcs[rank] = ent;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // R32: candidates of equal probability hold the same rank here, the smallest of their exact ranks, and wrote
            // the same entry: all but one of them find another lane's entry there (ent_lo: entries of different lanes
            // differ) and the ranks behind theirs hold stale data.  Only a KEPT rank is looked at: equal candidates share
            // their r32, so a tie inside the beam or across its boundary has every member below beam_size, and one wholly
            // below the boundary (PDQ: those candidates write as well) changes nothing the step uses.  Without a clash
            // every kept candidate's r32 IS its exact rank, every other candidate's exact rank is >= its r32 >= beam_size,
            // and no two of the table's first beam_size + 1 probability words are equal.
            // (Every lane reads, a lane that wrote nothing anywhere inside its half's table: the read-back then travels with
            // the table's other reads instead of waiting alone under a mask of its own.)
            if (R32) {
                const int back = srcs[PDQ ? rank : (rank & 15)];
                clash = sel && back != ent;
                if (HL) m_clash_t = m_sel & ballot(back != ent);
            }
            // (HL: its one look-up, `fate`, is written behind the table's reads, below -- the reads of neighbouring words are merged
            // only while no other LDS operation stands between them)
            if (!HL) {
            fate = HL ? __builtin_amdgcn_ds_bpermute(tgt_a, selflag) : bperm(hbase + mslot * GW, selflag);
            own = bperm(grp0, selflag);  // ... and this group's own candidate?
            }
            // every lane of new group i learns its source lane (stale beyond the new beam: unused), where the best
            // candidate sits, and the SMALLEST DEPTH in the new beam: a stale entry can only lower it
            if (HL) {
                // (the entries and the divisor first, in table order, ahead of every other LDS operation of the block: they
                // then come back as one ds_read_b128 and one ds_read2_b32)
                e_min = srcs[0];
#pragma unroll
                for (int j = 1; j < BCAP; ++j) e_min = min(e_min, srcs[j]);
                top = __int_as_float(srcs[kTop]);
            }
            const int e_src = srcs[PDQ ? i_src : i];
            src_a = e_src & (DSRC ? 0xFC : 0xFF);  // byte address, as ds_bpermute wants it
            if (!HL) e_min = srcs[0];
            top_a = e_min & 0xFF;
            if (DSRC) {
                // beam[0].probability() (:278) is rank 0's candidate probability: read off its sort key (read again by a
                // step that settles twice: a tie never changes rank 0's probability, but no register is trusted across
                // the rare block).  The gap quotient of the new slot waits on the source group's spare lane when the
                // source is a slot's own lane, and on the half's first idle lane (0 / top) when it is a child lane:
                // bit 0 of the entry says which.
                // (kRawTop: the word IS the probability, stored by the lane that held it)
                // (read behind the entries, below: the table then comes back as one ds_read_b128 and one ds_read2_b32)
                if (!kRawTop) top = key_prob((uint32_t)srcs[kTop]);
                if (HL) {
                    // a bit-field select: bit 0 spread over the word (v_bfe_i32) picks between the two addresses (v_bfi_b32).
                    // (Opaque: the optimiser otherwise rewrites it as v_and 1 / v_cmp_eq -> vcc / v_cndmask on vcc.)
                    int m_ch = (int)((uint32_t)e_src << 31) >> 31;
                    FCD_OPAQUE_VQ(m_ch);
                    gp_a = (m_ch & zero_a) | (~m_ch & (src_a + ((GW - 1) << 2)));
                    if (CHB) m_chw = m_ch;
                } else {
                    gp_a = (e_src & 1) ? zero_a : src_a + ((GW - 1) << 2);
                }
            }
            if (!HL) {
#pragma unroll
            for (int j = 1; j < BCAP; ++j) e_min = min(e_min, srcs[j]);
            }
            if (HL) {
                // (`own` is not looked up: "this group's own candidate was dropped" is a function of m_sel -- settle_gather)
                fate = __builtin_amdgcn_ds_bpermute(tgt_a, selflag);
                own = m_chw;  // (0 without CHB)
            }
            if (PDQ) {
                tie0 = (uint32_t)srcs[kTie + i_src];
                tie1 = (uint32_t)srcs[kTie + i_src + 1];
            }
        };
        // CHB: where the new slot's child entry is gathered from, picked by the same spread bit as gp_a.  The bit is set exactly
        // on the entries of child lanes (ent_lo, beam_wave.hip; a candidate sits on a slot's own lane or on a child lane, checked
        // at the top of the step), and a child lane's candidate -- a node entering the beam for the first time, or one coming
        // back, whose row the reload block below fetches -- hands over a child entry of -1.  That is what the first lane of the
        // half holds in `child` at all times: a slot's own lane and a spare lane start with -1 and, here, only ever gather from
        // that lane or from the source group's own / spare lane.  A source that is a slot's own lane is read at the source
        // group's lane k as before.
        // (The spread bit leaves settle_table() in `own`, which the HL step does not look up and both lambdas already name, and
        // the address takes its place here, in a lambda of its own: a variable more in settle_table() or settle_gather() would
        // change their closures' layout, which reaches the code of every other instantiation.)
        auto child_source = [&]() __attribute__((always_inline)) {
            if (CHB) own = (own & hbase_a) | (~own & (src_a + (k << 2)));
        };
        settle_table();
        child_source();
        // What a candidate hands to its new slot is packed HERE, behind the survivor table's wave barrier: the barrier is
        // a scheduling boundary, and ahead of it these dozen instructions sit on the step's dependent chain in front of
        // the table's LDS round trip instead of under it (r06: +2.4 % of the kernel when they moved ahead of it in r04,
        // found by bisection on one box -- profiles/r06b_headline_bisect.txt).
        const int tipfc = is_self ? tipf : (k << 2);
        int statec = (CRF && !is_self) ? (GATHER ? ((state * NL) & s_mask) + l : (state * NL) % (S > 0 ? S : 1) + l)
                                             : state;  // :97
        int jumpc = HL ? select_on_pair(~self_m & ballot((depth & ((kSeg - 1) << kDsh)) == 0), lane, node, jump)  // (one select, on a mask)
                       : (is_self ? jump : ((depth % kSeg == 0) ? node : jump));
        // 0 self, 1 a child entering the beam for the first time, 2 a child that has been there before (EVER:
        // its row is in HBM); read off the entry BEFORE it is marked below
        const int kind = is_child ? 1 + ((child_in >> 30) & 1) : 0;
        // HL: kind and tip label of a child lane are one constant plus the entry's EVER bit.  (A lane that is neither a slot's
        // own nor a child lane holds no candidate: it is never a source, and what it packs here is never gathered.)
        int meta = HL ? (depc | (is_self ? tipf : kind1 + ((child_in >> 30) & 1))) : (kind | tipfc | (depc << 5));
        // DSRC: every lane divides what it holds, HERE, before the gather: a candidate lane its label probability, a
        // group's spare lane the gap probability of the slot's own candidate (it received the blank column like the
        // slot's own lane and computed the same sgp), the half's idle lanes 0 -- a child candidate's gap probability.
        if (DSRC) dv = spare ? sgp : (idle ? 0.0f : clp);
        auto settle_gather = [&]() __attribute__((always_inline)) {
            {
                // a child entry whose node is a beam entry follows it to its new slot (or learns it left);
                // a child entering the beam is marked EVER: from now on it may own children
                const int followed = (child_in & kStored) | (fate << kSlotShift);
                const int entered = id | kEver | (selflag << kSlotShift);
                const bool upd = go && is_child;
                if (HL) {
                    // two selects on masks: no exec region and no branch is spent on the entry
                    const uint64_t m_ent = child_m & m_sel;
                    child_s = lane_in(m_ent, lane) ? entered : child_in;
                    child_s = lane_in(child_m & m_ib, lane) ? followed : child_s;
                } else {
                    child_s = (upd && inbeam) ? followed : ((upd && sel) ? entered : child_in);
                }
                // A node's child row only has to exist in HBM while the node is OUT of the beam (it is read back if
                // the node re-enters, below): write it once, when the node is evicted -- four lanes, 16 contiguous
                // bytes.  And only if the node can come back at all: a node re-enters the beam as the extension of its
                // parent, so it needs a proper ancestor in the beam -- none exists once every beam entry is at least as
                // deep as the node, and then none ever will (its ancestors have left for good, top-down from the
                // root).  Three evicted rows in four are dead by this test and are never written.
                if (HL) {  // ONE exec region, its mask joined in scalar registers
                    // "This group's own candidate was dropped" without an LDS look-up of the own lane's selflag: the kept
                    // own candidates are the bits of m_sel on the slots' own lanes, GW * i of a half; times 2 + 4 + 8 + 16
                    // each lands on its group's child lanes GW * i + 1 .. + 4.  The bits sit GW = 6 apart and the multiplier
                    // spans four, so no two products meet and nothing carries; the last group reaches bit GW * (BCAP - 1) + 4
                    // of its 32-bit half.  Two s_mul_i32 and the complement under child_m for a ds_bpermute_b32, its wait
                    // and a vector compare.
                    static_assert(!HL || (GW == 6 && NL <= 4 && GW * (BCAP - 1) + 4 < 32 && HALF == 32),
                                  "the own-lane bits replicate onto the child lanes without collision or carry");
                    // (m_sel & ~child_m: a candidate lane that is no child lane is a slot's own.  Not "& self_m": this lambda
                    // would capture one variable more, and the closure's layout reaches the code of every other instantiation.)
                    const uint64_t m_kept0 = m_sel & ~child_m;
                    const uint64_t m_own1 = (uint64_t)((uint32_t)m_kept0 * 30u) | ((uint64_t)((uint32_t)(m_kept0 >> 32) * 30u) << 32);
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: the multiple against its definition, group by group)
                    {
                        uint64_t by_group = 0ull;
                        for (int h = 0; h < 2; ++h)
                            for (int g = 0; g < BCAP; ++g)
                                if ((m_kept0 >> (32 * h + GW * g)) & 1ull) by_group |= 0x1Eull << (32 * h + GW * g);
                        if (by_group != m_own1) {
                            fprintf(stderr, "beam_wave: own-candidate bits %016llx replicate to %016llx, not %016llx\n",
                                    (unsigned long long)m_kept0, (unsigned long long)m_own1, (unsigned long long)by_group);
                            abort();
                        }
                    }
#endif
                    const uint64_t m_evict = (WSC ? m_cgrp : (child_m & m_grp)) & ~m_own1;
                    // (named, not read: the lambda captures its variables in the order it names them, and that order reaches
                    // the register allocation of every other instantiation.  `own` stood here.)
                    (void)own;
                    if (lane_in(m_evict & ballot(depth > e_min), lane))
                        *at32(rows_w, (hoff + (uint32_t)(node + 1)) * RW + l) = child_s;
                } else {
                const bool dead = (depth << 8) <= e_min;  // e_min = (minimum depth << 8) | a lane address
                if (upd && grp && own == 0 && !dead)
                    *at32(rows_w, (hoff + (uint32_t)(node + 1)) * RW + l) = child_s;  // (beam-position bits and all: stripped when read back)
                }
            }
            stamp_i(4, child_s);  // fate of every child entry, row eviction
            // ---- gather the survivors into rank order ----
            if (DSRC) {
                // the gathers that do not wait for the division travel under it; what is gathered last are the two
                // IEEE quotients themselves (:279-282) -- the new slot's label and gap probability, final
                n_meta = __builtin_amdgcn_ds_bpermute(src_a, meta);
                n_node = __builtin_amdgcn_ds_bpermute(src_a, id);
                n_state = CRF ? __builtin_amdgcn_ds_bpermute(src_a, statec) : 0;
                n_jump = __builtin_amdgcn_ds_bpermute(src_a, jumpc);
                n_child = __builtin_amdgcn_ds_bpermute(CHB ? own : src_a + (k << 2), child_s);  // (without CHB: meaningful when the source is a self lane)
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: the gather without CHB, for the check in kinds())
                n_child_kind = __builtin_amdgcn_ds_bpermute(src_a + (k << 2), child_s);
#endif
                stamp_i(5, n_meta);  // survivors gathered into rank order
                const float quot = dv / top;
                n_lp = __int_as_float(__builtin_amdgcn_ds_bpermute(src_a, __float_as_int(quot)));
                n_gp = __int_as_float(__builtin_amdgcn_ds_bpermute(gp_a, __float_as_int(quot)));
            } else {
            n_node = __builtin_amdgcn_ds_bpermute(src_a, id);
            n_lp = __int_as_float(__builtin_amdgcn_ds_bpermute(src_a, __float_as_int(clp)));
            n_gp = __int_as_float(__builtin_amdgcn_ds_bpermute(src_a, __float_as_int(cgp)));
            n_meta = __builtin_amdgcn_ds_bpermute(src_a, meta);
            n_state = CRF ? __builtin_amdgcn_ds_bpermute(src_a, statec) : 0;
            n_jump = __builtin_amdgcn_ds_bpermute(src_a, jumpc);
            n_child = __builtin_amdgcn_ds_bpermute(src_a + (k << 2), child_s);  // meaningful when the source is a self lane
            top = __int_as_float(__builtin_amdgcn_ds_bpermute(top_a, __float_as_int(prob)));  // beam[0].probability() :278 = its candidate's label + gap probability
            stamp_f(5, n_lp);  // survivors gathered into rank order
            }
        };
        settle_gather();
        int n_kind;
        bool reload;
        // (CHB: n_child arrives final -- the gather's address has looked at the source, so nothing here looks at its kind)
        auto kinds = [&]() __attribute__((always_inline)) {
            n_kind = n_meta & 3;
            if (CHB) {
            } else if (n_kind == 1 || !is_child) n_child = -1;
            reload = go && i < Bn && n_kind == 2 && is_child;
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: CHB against the look at the kind, on every lane of a running group
                   // that the reload block does not overwrite)
            if (CHB && !idle && i < Bn && !reload && n_child != ((n_kind == 1 || !is_child) ? -1 : n_child_kind)) {
                fprintf(stderr, "beam_wave: lane %d gathered the child entry %08x, the source's kind %d says %08x\n", lane,
                        (unsigned)n_child, n_kind, (unsigned)((n_kind == 1 || !is_child) ? -1 : n_child_kind));
                abort();
            }
#endif
        };
        kinds();
        // Two rare things share ONE branch (every instruction and, more so, every wait added to the step shows in the
        // kernel time): a node that was in the beam before comes back (kind 2: its child row is in HBM; the vote is on the
        // bare compare), and -- PDQ -- ranks i and i + 1 hold one probability, rank i is kept and rank i + 1 exists:
        // sort_unstable_by's order of the two is pdqsort's business once the list is longer than 20 (:262).  tie_lim
        // folds "i < beam_size", "i + 1 < n_valid" and "n_valid > 20" into one compare: equal probabilities among FEW
        // candidates are common on peaky posteriors (a third of such reads meet one) and must not take the QUICKSORT'S path.
        // (R32 takes the branch for them, to recount: 0.5 % of a wavefront's steps on peaky rows, one step in 512 000 on the
        // benchmark's -- DESIGN.md section 4 -- each for some 60 instructions and the second settling.)
        // (A half that is not running, or has just failed, has no candidates or loses nothing by re-ranking them.)
        // Masks, not lane flags: a flag used again inside the rare block would be materialised in a register.
        const uint64_t m_k2 = ballot(n_kind == 2);
        // R32: a third -- kept candidates of equal probability met in the survivor table.  The halves recount their EXACT
        // ranks from the two word tables (rank = #(greater probability word) + #(equal word, greater node word): an empty
        // slot's words are 0, 0 and count for nobody; a lane's own neither) and settle again; nothing of the first pass was
        // committed.  (Its eviction stores: `own`, `fate` and e_min came from a table with a hole -- a store it made that
        // the second pass does not is the harmless one described above, and one it skipped the second pass makes.)  The
        // PDQ hint needs no first-pass test at all: two equal words among the first beam_size + 1 ranks ARE a clash, so it is
        // read off the settled table, where no hole can raise or hide it.
        // HL: a fourth -- a candidate whose probability word is outside the range on which the f32 count is exact (device_utils.h,
        // fcd_rankf_outside: below 2^-76 and not 0, above 2^27, negative, a NaN).  The same recount: it is valid for every
        // input and replaces whatever the first pass counted.
        const uint64_t m_clash = R32 ? (HL ? (m_clash_t | m_guard) : ballot(clash)) : 0ull;
        const uint64_t m_hint = (PDQ && !R32) ? (ballot(tie0 == tie1) & ballot(tie_lim < n_valid)) : 0ull;
        if (__builtin_expect((m_k2 | m_hint | m_clash) != 0ull, 0)) {
            uint64_t m_tied = m_hint;
            if (WSC) {
                // the per-lane count as the first rare block left it: the count of a half that runs, 0 for one that does not or
                // has just failed (alive_m).  (From an opaque word, like the first block's: otherwise it is formed in every step.)
                uint32_t half_w = hbase ? (uint32_t)(m_valid >> 32) : (uint32_t)m_valid;
                FCD_OPAQUE_V(half_w);
                n_valid = lane_in(alive_m, lane) ? __builtin_popcount(half_w) : 0;
            }
            if (R32 && m_clash != 0ull) {
                if (RAWK) {
                    // The recount, the PDQ hint's list builder, the quicksort replay and the read-back of `key` behind it
                    // work on KEYED tables: every lane forms its keyed probability word (make_key_canonical's high word of
                    // pcanon; 0 without a candidate) and its node word HERE and writes both, one two-word write, as the
                    // top of the step did before.  The next step's top overwrites the probability table with raw words
                    // again, so two tied steps in a row each rebuild; a step that is here for a returning node only
                    // (m_k2) rebuilds nothing and reads neither table.
                    // The node word is taken from `id` -- a slot's own node, or the id field of the child entry as the
                    // step sees it, a new node's REAL id included.  Only the ORDER of node words is read (the recount and
                    // the list builder count the larger ones), and a new id exceeds every existing one and grows with the
                    // lane exactly as tks + q does (see the comment on the key's node index above).
                    key = valid ? make_key_canonical(__int_as_float(pword), id) : 0ull;
                    kwords[kslot] = (uint32_t)(key >> 32);
                    kwords[kslot + kNodeTab] = (uint32_t)key;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                const uint32_t kp = (uint32_t)(key >> 32);  // (RAWK: the keyed word, not the raw one of the first pass)
                const uint32_t kn = (uint32_t)key;
                int ex = 0;
#pragma unroll 1
                for (int ii = 0; ii < BCAP; ++ii) {  // a beam slot's N candidates per trip
                    uint32_t pu[N], nu[N];
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        pu[c] = kwords[hw + ii * N + c];
                        nu[c] = kwords[hw + ii * N + c + kNodeTab];
                    }
#pragma unroll
                    for (int c = 0; c < N; ++c) ex += (pu[c] > kp || (pu[c] == kp && nu[c] > kn)) ? 1 : 0;
                }
                rank = ex;
                settle_table();
                child_source();
                settle_gather();
                kinds();
                if (PDQ) m_tied = ballot(tie0 == tie1) & ballot(tie_lim < n_valid);
            }
            if (PDQ) {
                // Nothing of the step is committed yet: the ranks are replaced by the quicksort's (pdq178_wave.h) and
                // everything that depends on them runs again.  (An eviction store of the first pass that the second does
                // not repeat leaves a row in HBM nobody reads before it is written again: rows are read back only after
                // their node's LAST eviction.)
                if (m_tied != 0ull) {
                    const bool mine = RPW == 1 ? true : (hbase ? (m_tied >> 32) != 0ull : (uint32_t)m_tied != 0u);
                    __builtin_amdgcn_s_setprio(3);  // (a straggler in the making keeps the issue priority: see beam_lane.hip)
                    // (the lane and wavefront numbers as the rare block sees them: opaque copies, so that the dozen LDS
                    // addresses and lane masks the quicksort derives from them are formed HERE -- hoisted out of the time
                    // loop they were carried through it, and at five wavefronts per SIMD spilled)
                    int lane_r = lane, wave_r = wave;
                    if (PARK || RSORT) {
                        FCD_OPAQUE_V(lane_r);
                        FCD_OPAQUE_V(wave_r);
                    }
                    const int q_r = lane_r & (HALF - 1), hbase_r = lane_r - q_r;
                    uint64_t *list = s_list[wave_r] + hbase_r;
                    int *newrank = s_heads[wave_r];  // (free until the traceback)
                    // the list sort_unstable_by is handed: the merged candidates in ascending node order (:245-260)
                    int pos = 0;
                    if (RPW == 1) {
                        // one candidate per lane: every candidate lane's node word by v_readlane (three instructions per
                        // candidate, no memory; an empty slot's word is 0 and exceeds nothing)
#pragma unroll
                        for (int u = 0; u < NC; ++u) {
                            const uint32_t ou = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, (u / N) * GW + (u % N));
                            pos += ou > (uint32_t)key ? 1 : 0;  // low word: larger = smaller node
                        }
                    } else {
#pragma unroll 1
                    for (int ii = 0; ii < BCAP; ++ii) {  // a beam slot's N keys per trip: their loads travel together
                        if (R32) {  // the node table (an empty slot's word is 0 and exceeds nothing)
                            const uint32_t *nt = reinterpret_cast<const uint32_t *>(s_keys[wave_r]) + (hbase_r ? kHalfW : 0) + kNodeTab;
                            uint32_t nu[N];
#pragma unroll
                            for (int c = 0; c < N; ++c) nu[c] = nt[ii * N + c];
#pragma unroll
                            for (int c = 0; c < N; ++c) pos += nu[c] > (uint32_t)key ? 1 : 0;  // larger = smaller node
                            continue;
                        }
                        uint64_t ku[N];
#pragma unroll
                        for (int c = 0; c < N; ++c) ku[c] = s_keys[wave_r][hbase_r + ii * GW + c];
#pragma unroll
                        for (int c = 0; c < N; ++c)
                            pos += (ku[c] != 0ull && (uint32_t)ku[c] > (uint32_t)key) ? 1 : 0;  // low word: larger = smaller node
                    }
                    }
                    if (RPW == 1) {
                        // One read per wavefront (beams 6 .. 12): the list never goes to memory.  Every candidate pushes its
                        // probability word and its lane to lane `pos` (ds_permute: the list in node order, one element per
                        // lane), the quicksort runs in registers (pdq178_reg.h), and position j hands its rank back to
                        // the lane its element came from.  (At most 62 candidates: lane 63 takes what has nothing to say.)
                        static_assert(RPW != 1 || NC <= 62, "lane 63 is the idle target of the pushes");
                        const bool cand = key != 0ull;
                        uint32_t rk = (uint32_t)perm(cand ? pos : 63, (int)(uint32_t)(key >> 32));
                        uint32_t rt = (uint32_t)perm(cand ? pos : 63, lane);
                        const int n_list = __builtin_amdgcn_readfirstlane(n_valid);
                        pdq178::reg_sort(rk, rt, n_list, beam_size, false, 0u, 32 - __builtin_clz((unsigned)n_list), true, true,
                                         s_list[wave], lane);
                        const int back = perm(lane < n_list ? (int)rt : 63, lane);
                        if (cand) rank = back;
                    } else if (RSORT) {
                        // Two reads per wavefront, equal lengths (the headline): a half never holds more than BCAP * N
                        // candidates, so its list fits the lanes of the wavefront and the quicksort runs in registers, as
                        // above -- one flagged half after the other, the list of half hs in lanes 0 .. n_list - 1.  No list
                        // in LDS and no partition path through it.
                        // What the quicksort does not touch and the second settling (or the next step) needs waits in LDS
                        // meanwhile, so that the replay does not set the register budget of the whole kernel.
                        static_assert(!RSORT || NC <= 62, "lane 63 is the idle target of the pushes");
                        int *const park = s_park[RPARK ? wave_r : 0] + lane_r;
                        if (RPARK) {
#pragma unroll
                        for (int j = 0; j < kFifo; ++j) park[64 * j] = __float_as_int(win[j]);
                        park[64 * kFifo] = __float_as_int(incoming);
                        park[64 * (kFifo + 1)] = __float_as_int(dv);  // (all the second settle needs of clp, cgp and prob)
                        park[64 * (kFifo + 2)] = meta;
                        park[64 * (kFifo + 3)] = jumpc;
                        park[64 * (kFifo + 4)] = id;
                        park[64 * (kFifo + 5)] = child_in;
                        park[64 * (kFifo + 6)] = node;
                        park[64 * (kFifo + 7)] = depth;
                        park[64 * (kFifo + 8)] = statec;
                        }
#pragma unroll 1
                        for (int hs = 0; hs < RPW; ++hs) {
                            const bool flagged = (hs ? (m_tied >> 32) != 0ull : (uint32_t)m_tied != 0u);
                            if (!flagged) continue;
                            const bool cand = key != 0ull && (lane_r >= HALF) == (hs != 0);
                            uint32_t rk = (uint32_t)perm(cand ? pos : 63, (int)(uint32_t)(key >> 32));
                            uint32_t rt = (uint32_t)perm(cand ? pos : 63, lane_r);
                            const int n_list = __builtin_amdgcn_readlane(n_valid, hs * HALF);
                            pdq178::reg_sort<NC>(rk, rt, n_list, beam_size, false, 0u, 32 - __builtin_clz((unsigned)n_list), true, true,
                                                 s_list[wave_r], lane_r);
                            const int back = perm(lane_r < n_list ? (int)rt : 63, lane_r);
                            if (cand) rank = back;
                        }
                        if (RPARK) {
#pragma unroll
                        for (int j = 0; j < kFifo; ++j) win[j] = __int_as_float(park[64 * j]);
                        incoming = __int_as_float(park[64 * kFifo]);
                        dv = __int_as_float(park[64 * (kFifo + 1)]);
                        meta = park[64 * (kFifo + 2)];
                        jumpc = park[64 * (kFifo + 3)];
                        id = park[64 * (kFifo + 4)];
                        child_in = park[64 * (kFifo + 5)];
                        node = park[64 * (kFifo + 6)];
                        depth = park[64 * (kFifo + 7)];
                        statec = park[64 * (kFifo + 8)];
                        }
                        // the lane's own key, from the two word tables it wrote at the top of the step (a lane without a
                        // candidate reads the idle word: 0, 0; RAWK: the tables the recount above wrote KEYED in this very block
                        // -- m_tied is set only behind it -- so the second settling reads a key, never a raw word)
                        if (R32) key = ((uint64_t)kwords[kslot] << 32) | kwords[kslot + kNodeTab];
                        if (kRawTop) pword = __float_as_int(key_prob((uint32_t)(key >> 32)));
                    } else {
                    if (mine && key != 0ull) list[pos] = (key & 0xFFFFFFFF00000000ull) | (uint32_t)lane_r;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    // two reads per wavefront: the whole wavefront replays the quicksort on a flagged half's list, one half
                    // after the other (pdq178_wave.h; both halves flagged in the same step is rarer still)
                    // The quicksort is inlined and must not set the register budget of the whole kernel: what it does not
                    // touch -- the row FIFO, the prefetched row values and what the candidates hand to their new slots --
                    // waits in LDS meanwhile (as in beam_lane.hip).
                    int *const park = s_park[PARK ? wave_r : 0] + lane_r;
                    if (PARK) {
#pragma unroll
                        for (int j = 0; j < kFifo; ++j) park[64 * j] = __float_as_int(win[j]);
                        park[64 * kFifo] = __float_as_int(incoming);
                        park[64 * (kFifo + 1)] = __float_as_int(pk_next);
                        park[64 * (kFifo + 2)] = __float_as_int(ptip_next);
                        park[64 * (kFifo + 3)] = __float_as_int(dv);  // (all the second settle needs of clp, cgp and prob)
                        park[64 * (kFifo + 4)] = meta;
                        park[64 * (kFifo + 5)] = jumpc;
                        park[64 * (kFifo + 6)] = id;
                        park[64 * (kFifo + 7)] = child_in;
                        park[64 * (kFifo + 8)] = statec;
                        park[64 * (kFifo + 9)] = node;
                        park[64 * (kFifo + 10)] = depth;
                        park[64 * (kFifo + 11)] = tipf;
                        park[64 * (kFifo + 12)] = state;
                        park[64 * (kFifo + 13)] = (int)(uint32_t)key;
                        park[64 * (kFifo + 14)] = (int)(uint32_t)(key >> 32);
                        park[64 * (kFifo + 15)] = rank;
                    }
#pragma unroll 1
                    for (int hs = 0; hs < RPW; ++hs) {
                        const bool flagged = (hs ? (m_tied >> 32) != 0ull : (uint32_t)m_tied != 0u);
                        if (!flagged) continue;
                        const int len_h = __builtin_amdgcn_readlane(n_valid, hs * HALF);
                        pdq178::wave_sort_inline<1>(s_list[wave_r] + hs * HALF, len_h, beam_size, &s_ws[wave_r], lane_r);
                    }
                    if (PARK) {
#pragma unroll
                        for (int j = 0; j < kFifo; ++j) win[j] = __int_as_float(park[64 * j]);
                        incoming = __int_as_float(park[64 * kFifo]);
                        pk_next = __int_as_float(park[64 * (kFifo + 1)]);
                        ptip_next = __int_as_float(park[64 * (kFifo + 2)]);
                        dv = __int_as_float(park[64 * (kFifo + 3)]);
                        meta = park[64 * (kFifo + 4)];
                        jumpc = park[64 * (kFifo + 5)];
                        id = park[64 * (kFifo + 6)];
                        child_in = park[64 * (kFifo + 7)];
                        statec = park[64 * (kFifo + 8)];
                        node = park[64 * (kFifo + 9)];
                        depth = park[64 * (kFifo + 10)];
                        tipf = park[64 * (kFifo + 11)];
                        state = park[64 * (kFifo + 12)];
                        rank = park[64 * (kFifo + 15)];
                        key = (uint64_t)(uint32_t)park[64 * (kFifo + 13)] | ((uint64_t)(uint32_t)park[64 * (kFifo + 14)] << 32);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (PARK) {  // (formed again rather than kept across the quicksort)
                        FCD_OPAQUE_V(lane_r);
                        FCD_OPAQUE_V(wave_r);
                    }
                    const int q_s = lane_r & (HALF - 1);
                    const uint64_t *list_s = s_list[wave_r] + (lane_r - q_s);
                    newrank = s_heads[wave_r];
                    if (mine && q_s < n_valid) newrank[(int)(uint32_t)list_s[q_s]] = q_s;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (mine && key != 0ull) rank = newrank[lane_r];
                    }
                    settle_table();
                    child_source();
                    settle_gather();
                    kinds();
                }
            }
            if (ballot(n_kind == 2) != 0ull) {  // (again: the ranks may have changed)
                int e = -1;
                if (reload) e = load_i32_l2(at32(rows_w, (hoff + (uint32_t)(n_node + 1)) * RW + l));
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: device memory arrives poisoned with 0xA5)
                if (reload && e == (int)0xA5A5A5A5) {  // a row that was never written: the dead-row test (above) was wrong
                    fprintf(stderr, "beam_wave: node %d re-entered the beam but its child row was never stored\n", n_node);
                    abort();
                }
#endif
                if (e >= 0) e &= kStored;  // the stored entry still carries the beam-position bits it had at eviction
#pragma unroll
                for (int j = 0; j < BCAP; ++j) {
                    const int nj = bperm(hbase + j * GW, n_node);
                    if (reload && e >= 0 && j < Bn && (e & kIdMask) == nj)
                        e = (e & kStored) | kInBeam | (j << kSlotShift);
                }
                if (reload) n_child = e;
            }
        }
        if (AMB) {
            // [0] a kept candidate that shares its probability with any other candidate of a > 20-candidate step;
            // [1] (any candidate count) equal probabilities at ranks 0 / 1 or across the truncation boundary:
            //     the group of n_eq equal candidates occupies ranks [n_gt, n_gt + n_eq)
            const bool tie = sel && n_valid > 20 && n_eq >= 2;
            const bool crit = valid && go && n_eq >= 2 && (n_gt == 0 || (n_gt < beam_size && n_gt + n_eq > beam_size));
            const uint64_t m_tie = ballot(tie), m_crit = ballot(crit);
            n_amb += (RPW == 1 ? m_tie : (hbase ? (m_tie >> 32) : (m_tie & 0xFFFFFFFFull))) != 0ull ? 1 : 0;
            n_crit += (RPW == 1 ? m_crit : (hbase ? (m_crit >> 32) : (m_crit & 0xFFFFFFFFull))) != 0ull ? 1 : 0;
        }
        if (CRF && (UNI || go)) state = n_state;  // < S: (s*4) % 4 + l = l for (N, S) = (5, 4); masked when GATHER
        if (UNI || go) tipf = n_meta & 0x1C;
        if (GATHER) rowv = gather_row(t + 1);  // in flight during the divisions below (DSRC: behind the quotients' gather)
        else fetch_row(pk_next, ptip_next);    // (the FIFO was already advanced to step t + 1 above)
        float q_lp, q_gp;
        if (DSRC) {  // divided at the source, before the gather
            q_lp = n_lp;
            q_gp = n_gp;
        } else {
            // Every lane of a group would compute the same two IEEE quotients: lane k = 1 divides the gap
            // probability, the others the label probability -- one division per lane -- and the group shares them.
            const float quot = (k == 1 ? n_gp : n_lp) / top;
            q_lp = bpermf(grp0, quot);
            q_gp = bpermf(grp0 + 1, quot);
        }
        if (UNI || go) {
            node = n_node;
            lp = q_lp;
            gp = q_gp;
            depth = HL ? (n_meta & ~0xFF) : (n_meta >> 5);  // (HL: still shifted up by 8)
            jump = n_jump;
            child = n_child;
            if (!WSC) B = Bn;
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: the per-lane width, formed from the count as without WSC, for the check
                   // of the carried scalar state at the top of the next step)
            if (WSC) {
                const int n_now = lane_in(alive_m, lane) ? __builtin_popcount(hbase ? (uint32_t)(m_valid >> 32) : (uint32_t)m_valid) : 0;
                B = n_now < beam_size ? n_now : beam_size;
            }
#endif
        }
        stamp_f(6, lp);  // row reload, top, the two divisions, state update
