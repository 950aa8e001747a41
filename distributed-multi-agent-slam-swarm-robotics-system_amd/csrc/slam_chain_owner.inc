// The owner wave's loop over its chunks of events (qs_slam_chain_free_kernel, slam.hip): included there twice, with LEAN true
// (32-bit node indices, decisions settled by their first rows where that is possible) and false (the general owner).
// Everything it names is the kernel's.
        for (unsigned int q0 = e0; q0 < e1; q0 += QS_WAVE) {
            const int ag = ag_n, type = type_n;
            const long long idx = idx_n, next_first = nf_n;
            const double px = px_n, py = py_n;
            if (q0 + QS_WAVE < e1) load_chunk(q0 + QS_WAVE, ag_n, idx_n, type_n, px_n, py_n, nf_n);
            const unsigned long long own = __ballot(ag == a);
            unsigned long long done = 0;                                            // own lanes decided so far
            unsigned long long posted = 0;                                          // own lanes whose landmark pose is in the pending ring
            // own events up to lane hi (with the agent's drift as it is now: the events since its last closure)
            auto post_upto = [&](int hi) {
                if (!POST) return;
                const unsigned long long m = own & ~posted & ((2ull << hi) - 1);
                if ((m >> lane) & 1) {
                    const unsigned int ps = (q0 - e0 + (unsigned int)lane) % FR_PEND;
                    p_x[ps] = raw_pose ? px : px + c_dx; p_y[ps] = raw_pose ? py : py + c_dy;   // rx += cdx  :856-857
                }
                LDS_CBAR();
                if ((m >> lane) & 1) LDS_ST_RLX(&p_node[(q0 - e0 + (unsigned int)lane) % FR_PEND], idx);
                posted |= m;
            };
            // the chunk's slots of the closure ring (and, with POST, of the shorter pending ring, which then sets the distance):
            // their last holders are committed, read and cleared.  s_prog stands at this chunk's first node here.
            static_assert(FR_PEND <= FR_HAND && (FR_HAND & (FR_HAND - 1)) == 0, "ring depths");
            if (own) FR_SPIN(q0 - e0 + QS_WAVE > LDS_RLX(&s_comm) + ((POST ? (unsigned int)FR_PEND : HD) - QS_WAVE));
            // the events that may close a loop (:304: their agent is past its cool-down); the ones before the first need no decision
            // (lean: idx >= c_last + min_between on the low words -- the sum is clamped to [0, 2^31 - 1] first: an own lane's index is
            // in [0, 0x7f7f7f7f), so either clamp leaves the comparison what it was)
            const int idx32 = (int)idx;
            auto eligible = [&]() -> unsigned long long {
                if constexpr (LEAN) {
                    const long long t = c_last + min_between;
                    const int thr = __builtin_amdgcn_readfirstlane(t < 0 ? 0 : t > 0x7fffffffll ? 0x7fffffff : (int)t);
                    return own & ~done & __ballot(idx32 >= thr);
                }
                return own & ~done & __ballot(idx - c_last >= min_between);
            };
            unsigned long long elig = eligible();
            // A decision: (event f of the chunk, its pose with the agent's drift as it is NOW, the first nodes of its nine buckets,
            // their rows on the way).  The rows of the NEXT decision are asked for as soon as this one's closure is known -- before
            // the hand-over to the committer, whose LDS traffic then runs in the shadow of the loads.
            int f = 0, qtype = 0;
            long long qidx = 0, fr_rows = 0;
            double qx = 0, qy = 0;
            unsigned int node0 = 0;
            FqRows rows = {LL_MAX, LL_MAX, 0, 0, 0u};
            auto start_decision = [&](unsigned long long e_) {
                // (the frontier first: the rows are asked for after it is read -- an older value is only more cautious)
                fr_rows = LDS_RLX(&s_frontier);
                f = __ffsll((long long)e_) - 1;
                post_upto(f);
                qidx = rl64(idx, f);
                const double spx = rlf64(px, f), spy = rlf64(py, f);
                qx = raw_pose ? spx : spx + c_dx; qy = raw_pose ? spy : spy + c_dy;               // rx += cdx  :856-857
                qtype = __builtin_amdgcn_readlane(type, f);
                int qcx, qcy;
                node0 = fq_node0(bg, qx, qy, qtype, lane, qcx, qcy);
                __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                fq_load(g_nodes, g_next, node0, lane, rows);
            };
            // The same for the lean owner: the index's low word only (an empty slot reads 0x7f7f7f7f, above every index there
            // is; no node: INT_MAX), no second load for the node's last index (the decision takes it from a ballot), one 32-bit
            // byte offset from the table's base, the hash from the lane's constants.  And the side list's length as of the
            // frontier just read (read after it: not older): a decision is only settled by its first rows while that is 0.
            int rid32 = 0x7fffffff, rla32 = 0x7fffffff;                              // (rla32: the node's look-ahead word, slam_chain_decide.inc)
            long long nm_rows = 0;
            auto start_decision_lean = [&](unsigned long long e_) {
                fr_rows = LDS_RLX(&s_frontier);
                LDS_CBAR();
                nm_rows = s_nmisc;
                f = __ffsll((long long)e_) - 1;
                post_upto(f);
                qidx = (long long)__builtin_amdgcn_readlane(idx32, f);
                const double spx = rlf64(px, f), spy = rlf64(py, f);
                qx = spx + c_dx; qy = spy + c_dy;                                                   // rx += cdx  :856-857
                qtype = __builtin_amdgcn_readlane(type, f);
                int qcx, qcy;
                const bool indexed = bucket_cell(qx, qy, qtype, bg, qcx, qcy);
                unsigned int h = ((unsigned int)qcx * 0x9E3779B1u + l_hx) ^ ((unsigned int)qcy * 0x85EBCA77u + l_hy);
                h ^= h >> 15;
                node0 = (indexed && l_in9) ? 1u + (unsigned int)(qtype - 1) * (bg.hmask + 1u) + (h & bg.hmask) : 0u;
                __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                rid32 = 0x7fffffff; rla32 = 0x7fffffff; rows.nx = 0; rows.ny = 0; rows.nxt = 0;
                if (node0) {
                    const QS_GLOBAL char *const row = (const QS_GLOBAL char *)g_nodes + (node0 * (unsigned int)sizeof(QsLmNode) + l_se8);
                    rid32 = *(const QS_GLOBAL int *)row;
                    rla32 = *(const QS_GLOBAL int *)((const QS_GLOBAL char *)g_nodes + (node0 * (unsigned int)sizeof(QsLmNode) + la_off));
                    rows.nx = *(const QS_GLOBAL double *)(row + offsetof(QsLmNode, x));
                    rows.ny = *(const QS_GLOBAL double *)(row + offsetof(QsLmNode, y));
                    rows.nxt = g_next[node0];
                }
            };
            // eff on 32 bits for the lean owner's decision (slam_chain_decide.inc): min(frontier as read before the rows, limit), negative: -1
            auto lean_eff32 = [&](long long limit_) -> int {
                const long long eff = fr_rows < limit_ ? fr_rows : limit_;
                return __builtin_amdgcn_readfirstlane(eff < 0 ? -1 : (int)eff);                       // (limit < 0x7f7f7f7f)
            };
            if (elig) { if constexpr (LEAN) start_decision_lean(elig); else start_decision(elig); }
            while (elig) {
#include "slam_chain_decide.inc"
                done |= (2ull << f_c) - 1;                                          // (lanes up to f: decided)
                double cdx = 0, cdy = 0;
                if (gbest != LL_MAX) {
                    const double ex = wx - qx_c, ey = wy - qy_c;                    // :311-312
                    cdx = ex * corr; cdy = ey * corr;                               // :314-315
                    c_dx += cdx; c_dy += cdy; c_last = qidx_c;                      // :911-914, :318
                }
                // the next decision, its rows on the way ...
                elig = eligible();
                if (elig) { if constexpr (LEAN) start_decision_lean(elig); else start_decision(elig); }
                // ... and this one handed over
                if (gbest != LL_MAX) {
                    // the closing event's slot (free since the top of the chunk): the payload, then the word that says "closes"
                    const unsigned int sl = (q0 - e0 + (unsigned int)f_c) % HD;
                    if (lane == 0) { d_cdx[sl] = cdx; d_cdy[sl] = cdy; d_ax[sl] = c_dx; d_ay[sl] = c_dy; }
                    LDS_CBAR();
                    if (lane == 0) LDS_ST_RLX(&d_midx[sl], gbest);
                }
                // decided: everything of this owner below its next event that may close (or, failing one in this chunk, below the
                // next chunk's first event)
                publish_prog(elig ? qidx : next_first);
            }
            post_upto(QS_WAVE - 1);                                                 // (the agent's events after its last decision of the chunk)
            publish_prog(next_first);
        }
