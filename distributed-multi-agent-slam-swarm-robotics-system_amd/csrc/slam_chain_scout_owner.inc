// The lean owner walking its agent's plan with a scout wave (qs_slam_chain_free_kernel<false, 8, false>, slam.hip; the scout:
// slam_chain_scout.inc): included there once, for graphs of up to two agents.  Everything it names is the kernel's.
// The walk is slam_chain_plan_owner.inc's.  What differs is where a decision's rows come from: the scout has staged, in LDS,
// the first nodes of a window of buckets around the pose it foresaw for this candidate two decisions ago.  If the stage is
// there, is for this candidate (the tag) and its window holds the 3 x 3 buckets of the real pose, the owner settles the
// decision from it: the lean decision's expressions (slam_chain_decide.inc), on up to FR_SC_K staged entries a lane, the lanes
// whose bucket is outside the 3 x 3 masked out, the limit on node indices from the frontier the SCOUT read ahead of its loads.
// A match with no bucket to walk further is final: the index holds a prefix in node order, complete up to any frontier read
// before the loads, so nothing below the match is missing from the rows, and a wider set of buckets cannot lower the first
// match -- the distance test decides.  Anything else -- no stage, another candidate, a window that misses, no match, a bucket
// to walk, a side list -- is the decision as it always was: the owner's own loads, then slam_chain_decide.inc.
// Decision number dec takes the stage of that number (parity dec & 1), made from the post after decision dec - 2: the owner reads
// a stage before it posts, and the scout writes a buffer only for a post it has seen, so a buffer is never written under a read.
        {
            constexpr bool LEAN = true;
            const unsigned int pl_b = (unsigned int)__builtin_amdgcn_readfirstlane((int)sb.agent_ev[bot0 + a]);
            const unsigned int n_own = (unsigned int)__builtin_amdgcn_readfirstlane((int)sb.agent_ev[bot0 + a + 1]) - pl_b;
            const QS_GLOBAL QsPlanRec *const pl = (const QS_GLOBAL QsPlanRec *)sb.pl_rec + pl_b;
            const unsigned int j_last = n_own ? n_own - 1 : 0u;                     // (a record that can always be asked for)
            unsigned int j = n_own ? (unsigned int)__builtin_amdgcn_readfirstlane((int)sb.pl_first[bot0 + a]) : 0u;
            unsigned int cur_r = 0, cur_skip = 0;
            unsigned int ahead = 0, ahead_of = ~0u;                                 // (the chunk of 64 records whose successor has been asked for)
            unsigned int comm_c = 0;                                                // s_comm as read last: it only grows
            auto ring_wait = [&]() {                                                // (slam_chain_plan_owner.inc)
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
            int qcx = 0, qcy = 0;
            bool indexed = false;
            unsigned int dec = 0;                                                   // decisions made so far: this one's number
            unsigned int st_staged = 0, st_fall = 0;
            // the lane's staged slots (slam_chain_scout.inc): slot lane + 64 k is an entry of window bucket (lane + 64 k) / 7, row-major
            unsigned int l_sbx[FR_SC_K], l_sby[FR_SC_K];
#pragma unroll
            for (int k = 0; k < FR_SC_K; k++) {
                const int b = (lane + QS_WAVE * k) / QS_NODE_CAP;
                const bool v = b < FR_SC_W * FR_SC_W;
                l_sbx[k] = v ? (unsigned int)(b % FR_SC_W) : 0x40000000u; l_sby[k] = v ? (unsigned int)(b / FR_SC_W) : 0x40000000u;
            }
            // the candidate's record c: what this decision asks (start_decision_plan's statements but for the rows)
            auto take_candidate = [&](const QsPlanRec &c) {
                cur_r = (unsigned int)__builtin_amdgcn_readfirstlane((int)c.r);
                cur_skip = (unsigned int)__builtin_amdgcn_readfirstlane((int)c.skip);
                qidx = (long long)__builtin_amdgcn_readfirstlane(c.node);
                qx = c.px + c_dx; qy = c.py + c_dy;                                                 // rx += cdx  :856-857
                qtype = c.type;
                indexed = bucket_cell(qx, qy, qtype, bg, qcx, qcy);
            };
            // the rows by the owner's own loads: the rest of start_decision_plan
            auto start_rows = [&]() {
                fr_rows = LDS_RLX(&s_frontier);
                LDS_CBAR();
                nm_rows = s_nmisc;
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
                const long long lim = qidx - (min_between > 1 ? min_between : 1), eff = fr_rows < lim ? fr_rows : lim;
                eff32_n = __builtin_amdgcn_readfirstlane(eff < 0 ? -1 : (int)eff);                 // (limit < 0x7f7f7f7f)
            };
            // the word for the scout: the next candidate and the drift it is queried with, then the post's number
            auto post_scout = [&]() {
                const unsigned int s = dec + 1u;
                if (lane == 0) { sc_j[a][s & 1u] = j; sc_dx[a][s & 1u] = c_dx; sc_dy[a][s & 1u] = c_dy; }
                LDS_CBAR();
                if (lane == 0) LDS_ST_RLX(&sc_word[a], s);
            };
            if (j < n_own) post_scout();
            while (j < n_own) {
                long long gb = LL_MAX; double w_x = 0, w_y = 0;
                bool settled = false;
                // ---- the candidate's record and rows: from the stage of this decision's number, if it is there and is for j ----
                const unsigned int p = dec & 1u;
                // every scout's part there?  (asked again FR_SC_WAIT times at the most: a stage that is late is not waited for)
                auto stage_ready = [&]() {
                    unsigned int r = 1u;
#pragma unroll
                    for (int q = 0; q < FR_SC_SPLIT; q++) r &= LDS_RLX(&sg_ready[a][p][q]) == dec ? 1u : 0u;
                    return __builtin_amdgcn_readfirstlane((int)r) != 0;
                };
                bool rdy = stage_ready();
                for (int t = 0; !rdy && t < FR_SC_WAIT; t++) rdy = stage_ready();
                bool have = false;
                int bcx = 0, bcy = 0, eff32s = -1;
                long long il[FR_SC_K]; double sx[FR_SC_K], sy[FR_SC_K];
#pragma unroll
                for (int k = 0; k < FR_SC_K; k++) { il[k] = 0; sx[k] = 0; sy[k] = 0; }
                QsPlanRec c = {0, 0u, 0, 0u, 0.0, 0.0};
                if (rdy) {
                    LDS_CBAR();
                    // (the scouts work alone: what they say about the stage has to agree, and the older frontier holds for all of it)
                    unsigned int tag = sg_tag[a][p][0];
                    bcx = sg_bcx[a][p][0]; bcy = sg_bcy[a][p][0]; eff32s = sg_eff[a][p][0];
#pragma unroll
                    for (int q = 1; q < FR_SC_SPLIT; q++) {
                        if (sg_tag[a][p][q] != tag || sg_bcx[a][p][q] != bcx || sg_bcy[a][p][q] != bcy) tag = ~0u;
                        eff32s = min(eff32s, sg_eff[a][p][q]);
                    }
                    c.node = sg_rnode[a][p]; c.r = sg_rr[a][p]; c.skip = sg_rskip[a][p]; c.type = sg_rtype[a][p];
                    c.px = sg_rpx[a][p]; c.py = sg_rpy[a][p];
#pragma unroll
                    for (int k = 0; k < FR_SC_K; k++) {
                        il[k] = sg_idla[a][p][lane + QS_WAVE * k]; sx[k] = sg_x[a][p][lane + QS_WAVE * k]; sy[k] = sg_y[a][p][lane + QS_WAVE * k];
                    }
                    have = (unsigned int)__builtin_amdgcn_readfirstlane((int)tag) == j;
                    bcx = __builtin_amdgcn_readfirstlane(bcx); bcy = __builtin_amdgcn_readfirstlane(bcy);
                    eff32s = __builtin_amdgcn_readfirstlane(eff32s);
                }
                if (!have) c = plan_rec(pl + j);                                    // (no stage for j: the record by the owner's own load)
                take_candidate(c);
                // decided: everything of this owner below this candidate -- the own events in between are inside the cool-down,
                // write nothing, and their slots stay LL_MAX
                publish_prog(qidx); ring_wait();
                if ((j >> 6) != ahead_of) {                                         // (the touch of the 64 records ahead: slam_chain_plan_owner.inc)
                    ahead_of = j >> 6;
                    __asm__ volatile("" :: "v"(ahead));
                    const unsigned int k = ((j & ~63u) + 64u) + (unsigned int)lane;
                    ahead = pl[k < j_last ? k : j_last].skip;
                }
                const unsigned int q0 = e0 + cur_r;                                 // (the event's place in the list, as the decision's text asks for it)
                if (have) {
                    // the 3 x 3 around the real cell inside the window: its lower corner at (ux, uy) from the window's base
                    const unsigned int ux = (unsigned int)qcx - 1u - (unsigned int)bcx, uy = (unsigned int)qcy - 1u - (unsigned int)bcy;
                    if (ux <= (unsigned int)(FR_SC_W - 3) && uy <= (unsigned int)(FR_SC_W - 3)) {
                        const int eff32 = eff32s;
                        bool inl[FR_SC_K], hit[FR_SC_K];
                        unsigned int v = 0xffffffffu;
#pragma unroll
                        for (int k = 0; k < FR_SC_K; k++) {
                            const int id = (int)(unsigned int)il[k];
                            const bool in9 = l_sbx[k] - ux <= 2u && l_sby[k] - uy <= 2u;
                            inl[k] = in9 && id <= eff32;
                            const double dx = qx - sx[k], dy = qy - sy[k];
                            hit[k] = inl[k] && dx * dx + dy * dy < r2thr;                  // :308-309
                            v = min(v, hit[k] ? (unsigned int)id : 0xffffffffu);
                        }
                        if (__ballot(v != 0xffffffffu)) {
                            const unsigned int g32 = wave_min_u32(v);
                            bool mo = false;
#pragma unroll
                            for (int k = 0; k < FR_SC_K; k++) mo = mo || (inl[k] && (int)(il[k] >> 32) < (int)g32);
                            if (__ballot(mo) == 0) {
                                const int w = __ffsll((long long)__ballot(v == g32)) - 1;
                                double selx = sx[0], sely = sy[0];
#pragma unroll
                                for (int k = 1; k < FR_SC_K; k++)
                                    if (hit[k] && (unsigned int)il[k] == g32) { selx = sx[k]; sely = sy[k]; }
                                gb = (long long)g32; w_x = rlf64(selx, w); w_y = rlf64(sely, w);
                                settled = true;
                            }
                        }
                    }
                }
                if (settled) st_staged++;
                else {
                    // ---- as it always was ----
                    st_fall++;
                    start_rows();
#include "slam_chain_decide.inc"
                    gb = gbest; w_x = wx; w_y = wy;
                }
                double cdx = 0, cdy = 0;
                if (gb != LL_MAX) {
                    const double ex = w_x - qx, ey = w_y - qy;                      // :311-312
                    cdx = ex * corr; cdy = ey * corr;                               // :314-315
                    c_dx += cdx; c_dy += cdy; c_last = qidx;                        // :911-914, :318
                    j = cur_skip;
                } else j++;                                                         // no closure: the agent's next event
                dec++;
                // the scout on its way to the candidate after the next one ...
                if (j < n_own) post_scout();
                // ... and this decision handed over
                if (gb != LL_MAX) {
                    // the closing event's slot (free: ring_wait, before anything was written for it): the payload, then the word that says "closes"
                    const unsigned int sl = cur_r % HD;
                    if (lane == 0) { d_cdx[sl] = cdx; d_cdy[sl] = cdy; d_ax[sl] = c_dx; d_ay[sl] = c_dy; }
                    LDS_CBAR();
                    if (lane == 0) LDS_ST_RLX(&d_midx[sl], gb);
                }
            }
            LDS_CBAR();
            if (lane == 0) LDS_ST_RLX(&sc_word[a], ~0u);                            // the scout may leave
            if (lane == 0 && (st_staged | st_fall)) { atomicAdd(scout_cnt, st_staged); atomicAdd(scout_cnt + 1, st_fall); }
        }
