// The lean owner walking its agent's plan (qs_slam_chain_free_kernel, slam.hip; the plan: qs_slam_plan_*_kernel): included there
// once, for the graphs that run the lean owner in a launch that has a plan.  Everything it names is the kernel's.
// Which event the agent queries next depends on a decision in one way only -- whether it closed: after a closure at own event j
// the agent's first event past the cool-down (skip[j], worked out before this kernel started), without one own event j + 1
// (eligible, since j was and the nodes ascend).  So the owner holds the record of its candidate, the same values in every
// lane, asks for the record at skip[j] right behind the rows of j, and between a match and the next request for rows does
// the closure, the pose, the cell and the hash: no chunk of the shared list, no ballot over it, no lane to read out.
        {
            constexpr bool LEAN = true;
            // (readfirstlane: the wave's number comes from threadIdx, so what follows from it is not known to be the same in every lane)
            const unsigned int pl_b = (unsigned int)__builtin_amdgcn_readfirstlane((int)sb.agent_ev[bot0 + a]);
            const unsigned int n_own = (unsigned int)__builtin_amdgcn_readfirstlane((int)sb.agent_ev[bot0 + a + 1]) - pl_b;
            const QS_GLOBAL QsPlanRec *const pl = (const QS_GLOBAL QsPlanRec *)sb.pl_rec + pl_b;
            const unsigned int j_last = n_own ? n_own - 1 : 0u;                     // (a record that can always be asked for)
            // the candidate: own event j (n_own: none left), its place in the graph's list, where a closure at it leads; the
            // record a closure leads to, asked for behind the candidate's rows
            unsigned int j = n_own ? (unsigned int)__builtin_amdgcn_readfirstlane((int)sb.pl_first[bot0 + a]) : 0u;
            unsigned int cur_r = 0, cur_skip = 0;
            QsPlanRec nxt = {0, 0u, 0, 0u, 0.0, 0.0};
            unsigned int ahead = 0, ahead_of = ~0u;                                 // (the chunk of 64 records whose successor has been asked for)
            unsigned int comm_c = 0;                                                // s_comm as read last: it only grows
            // The ring: the slot of position r is free once the committer has read and cleared its previous holder, r - HD.  The
            // owner keeps today's distance -- never further ahead of s_comm than HD - 64 events --, checked per candidate against
            // the value read last and read again only when that no longer suffices.  It waits with its progress word already at
            // the candidate's node, for events at least HD - 64 positions older than the candidate: all of them decided by owners
            // that nothing newer can hold back (their own ring waits point further back still, their frontier waits at the
            // committer, which needs nothing of this owner below its candidate), so it ends.
            auto ring_wait = [&]() {
                if (cur_r > comm_c + (HD - QS_WAVE)) {
                    comm_c = LDS_RLX(&s_comm);
                    if (cur_r > comm_c + (HD - QS_WAVE)) FR_SPIN(cur_r > (comm_c = LDS_RLX(&s_comm)) + (HD - QS_WAVE));
                }
            };
            int f = 0, qtype = 0;
            long long qidx = 0, fr_rows = 0;
            double qx = 0, qy = 0;
            unsigned int node0 = 0;
            FqRows rows = {LL_MAX, LL_MAX, 0, 0, 0u};
            int rid32 = 0x7fffffff, rla32 = 0x7fffffff;
            long long nm_rows = 0;
            int eff32_n = -1;
            auto lean_eff32 = [&](long long) -> int { return eff32_n; };
            // start_decision_lean's statements (slam_chain_owner.inc) on the candidate's record c; behind the rows, the record a
            // closure here leads to: it arrives in the shadow of the query.  (Everything of c is taken out before that record
            // is asked for, its place and its skip into scalar registers: nothing of c is live under the load, which can then
            // land in the registers c had -- a copy where the loop closes would wait for the loads just issued.)
            auto start_decision_plan = [&](const QsPlanRec &c) {
                fr_rows = LDS_RLX(&s_frontier);
                LDS_CBAR();
                nm_rows = s_nmisc;
                cur_r = (unsigned int)__builtin_amdgcn_readfirstlane((int)c.r);
                cur_skip = (unsigned int)__builtin_amdgcn_readfirstlane((int)c.skip);
                qidx = (long long)__builtin_amdgcn_readfirstlane(c.node);
                qx = c.px + c_dx; qy = c.py + c_dy;                                                 // rx += cdx  :856-857
                qtype = c.type;
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
                nxt = plan_rec(pl + (cur_skip < j_last ? cur_skip : j_last));
                // what the decision's text works out from the frontier and the limit (lean_eff32), here: under the loads
                const long long lim = qidx - (min_between > 1 ? min_between : 1), eff = fr_rows < lim ? fr_rows : lim;
                eff32_n = __builtin_amdgcn_readfirstlane(eff < 0 ? -1 : (int)eff);                 // (limit < 0x7f7f7f7f)
                // ... and, once per 64 records of the walk, the 64 after them, a lane each, for their cache lines: the plan was
                // written by other CUs, so a record comes from beyond the L2 -- further away than one query lasts, and the loop
                // waits for all its loads at every match.  Nothing of them is used; the empty statement stands for their use,
                // so that the load is kept, and is waited for no earlier than the next match.
                if ((j >> 6) != ahead_of) {
                    ahead_of = j >> 6;
                    __asm__ volatile("" :: "v"(ahead));
                    const unsigned int k = ((j & ~63u) + 64u) + (unsigned int)lane;
                    ahead = pl[k < j_last ? k : j_last].skip;
                }
            };
            if (j < n_own) {
                nxt = plan_rec(pl + j);
                publish_prog((long long)nxt.node);                                  // decided: everything of this owner below its first candidate
                start_decision_plan(nxt);
                ring_wait();
            }
            while (j < n_own) {
                const unsigned int q0 = e0 + cur_r;                                 // (the event's place in the list, as the decision's text asks for it)
#include "slam_chain_decide.inc"
                double cdx = 0, cdy = 0;
                const unsigned int r_c = cur_r;
                if (gbest != LL_MAX) {
                    const double ex = wx - qx_c, ey = wy - qy_c;                    // :311-312
                    cdx = ex * corr; cdy = ey * corr;                               // :314-315
                    c_dx += cdx; c_dy += cdy; c_last = qidx_c;                      // :911-914, :318
                    j = cur_skip;
                } else {
                    j++;                                                            // no closure: the agent's next event (rare: asked for now)
                    nxt = plan_rec(pl + (j < j_last ? j : j_last));
                }
                // the next decision, its rows on the way ...
                if (j < n_own) start_decision_plan(nxt);
                // ... and this one handed over
                if (gbest != LL_MAX) {
                    // the closing event's slot (free: ring_wait, before anything was written for it): the payload, then the word that says "closes"
                    const unsigned int sl = r_c % HD;
                    if (lane == 0) { d_cdx[sl] = cdx; d_cdy[sl] = cdy; d_ax[sl] = c_dx; d_ay[sl] = c_dy; }
                    LDS_CBAR();
                    if (lane == 0) LDS_ST_RLX(&d_midx[sl], gbest);
                }
                // decided: everything of this owner below its next candidate -- the own events in between are inside the cool-down,
                // write nothing, and their slots stay LL_MAX
                if (j < n_own) { publish_prog(qidx); ring_wait(); }
            }
        }
