// A scout wave of an owner of qs_slam_chain_free_kernel<false, 8, false> (slam.hip): included there once, for the graphs of up to two
// agents whose owners walk a plan (slam_chain_scout_owner.inc).  Everything it names is the kernel's; sc_o: its owner, sc_q: which
// of the owner's FR_SC_SPLIT scouts it is.
// After every decision the owner posts its next candidate j_next and its drift.  If that candidate closes, the one after it is
// c2 = skip[j_next], queried at p[c2] + drift + (the correction of the closure in between): less than half a bucket edge per axis
// with the reference's constants, so the 3 x 3 buckets of that query lie inside a window of FR_SC_W x FR_SC_W cells that is known now.
// The scouts read the first node of every bucket of that window -- the words the lean owner would ask for, by the same loads, behind
// the same read of the frontier -- and leave them in LDS, in the stage buffer of the post's parity, each its share of the slots
// and its own copy of what goes with them: the candidate they are for (the tag), the window's base cell and the decision's limit
// on node indices as of the frontier it read.  The owner takes them two decisions later, if the tag is its candidate and the
// 3 x 3 of the real pose is inside the window; whatever else happens it asks for its rows itself, as it always did.
// Nothing here has to be right for the owner's decision to be right but the rows, the limit and the tag, which all follow from
// the one word j_next: a drift read while the owner writes the next one moves the window, and the owner checks the window.
// Waits: for the owner's word only (FR_SPIN), which the owner moves after every decision and sets to "done" when it leaves.
        {
            const int o = sc_o;
            const unsigned int pl_b = (unsigned int)__builtin_amdgcn_readfirstlane((int)sb.agent_ev[bot0 + o]);
            const unsigned int n_own = (unsigned int)__builtin_amdgcn_readfirstlane((int)sb.agent_ev[bot0 + o + 1]) - pl_b;
            const QS_GLOBAL QsPlanRec *const pl = (const QS_GLOBAL QsPlanRec *)sb.pl_rec + pl_b;
            const unsigned int j_last = n_own ? n_own - 1 : 0u;
            const QsNodeG g_nodes = (QsNodeG)Gp->nodes;
            const QsU32G g_next = (QsU32G)Gp->nd_next;
            const int mb1 = min_between > 1 ? min_between : 1;
            // the lane's slots: slot s = lane + 64 k is entry s % 7 of the first node of window bucket s / 7 (row-major); its share
            // of the hash (as the lean owner's l_hx, l_hy, from the window's base cell), its entry's byte offset in a node row
            unsigned int s_hx[FR_SC_KW], s_hy[FR_SC_KW], s_se8[FR_SC_KW];
            int s_slot[FR_SC_KW];
            bool s_valid[FR_SC_KW], s_last[FR_SC_KW];
#pragma unroll
            for (int k = 0; k < FR_SC_KW; k++) {
                const int s = lane + QS_WAVE * (sc_q * FR_SC_KW + k), b = s / QS_NODE_CAP, e = s % QS_NODE_CAP;
                s_slot[k] = s;
                s_valid[k] = b < FR_SC_W * FR_SC_W;
                s_hx[k] = (unsigned int)(b % FR_SC_W) * 0x9E3779B1u; s_hy[k] = (unsigned int)(b / FR_SC_W) * 0x85EBCA77u;
                s_se8[k] = (unsigned int)e * 8u;
                s_last[k] = e == QS_NODE_CAP - 1;
            }
            unsigned int seen = 0;                                                  // the post dealt with last
            // the record staged last (its own index, its skip), and the record at that skip, asked for as soon as the stage is out:
            // where every decision closes, it is the next one to stage
            unsigned int pv_c2 = ~0u, pv_skip = 0, ah_c2 = ~0u;
            QsPlanRec ah = {0, 0u, 0, 0u, 0.0, 0.0};
            for (;;) {
                unsigned int w = seen;
                FR_SPIN((w = LDS_RLX(&sc_word[o])) == seen);
                if (w == seen || w == ~0u) break;                                   // (out of patience: never) / the owner has left
                LDS_CBAR();
                // the post, and the frontier: before the rows, as start_decision_plan reads it
                const unsigned int jn = (unsigned int)__builtin_amdgcn_readfirstlane((int)sc_j[o][w & 1u]);
                const double ddx = sc_dx[o][w & 1u], ddy = sc_dy[o][w & 1u];
                const long long fr = LDS_RLX(&s_frontier);
                LDS_CBAR();
                const long long nm = s_nmisc;
                seen = w;
                // (nothing to stage -- no candidate after the cool-down --: said at once, so that the owner does not ask again)
                auto nothing = [&]() {
                    if (lane == 0) sg_tag[o][w & 1u][sc_q] = ~0u;
                    LDS_CBAR();
                    if (lane == 0) LDS_ST_RLX(&sg_ready[o][w & 1u][sc_q], w);
                };
                if (jn >= n_own) { nothing(); continue; }
                const unsigned int c2 = jn == pv_c2 ? pv_skip : (unsigned int)__builtin_amdgcn_readfirstlane((int)pl[jn].skip);
                if (c2 >= n_own) { nothing(); continue; }
                QsPlanRec rec;
                if (c2 == ah_c2) rec = ah; else rec = plan_rec(pl + c2);
                pv_c2 = c2; pv_skip = (unsigned int)__builtin_amdgcn_readfirstlane((int)rec.skip);
                const double x = rec.px + ddx, y = rec.py + ddy;
                const int qtype = rec.type;
                int fcx, fcy;
                const bool indexed = bucket_cell(x, y, qtype, bg, fcx, fcy);
                // the window's base cell: the shift is under half a cell, so on either axis the real cell is this one or the one
                // on the side the pose is nearer to (4 x 4); or two cells either way (5 x 5).  The owner checks.
                int bcx = fcx - 2, bcy = fcy - 2;
                if (FR_SC_W == 4) {
                    const double tx = (x - bg.bx0) * bg.inv_cell, ty = (y - bg.by0) * bg.inv_cell;
                    if (!(tx - floor(tx) < 0.5)) bcx = fcx - 1;
                    if (!(ty - floor(ty) < 0.5)) bcy = fcy - 1;
                }
                __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                int id[FR_SC_KW], la[FR_SC_KW];
                double nx[FR_SC_KW], ny[FR_SC_KW];
#pragma unroll
                for (int k = 0; k < FR_SC_KW; k++) {
                    unsigned int h = ((unsigned int)bcx * 0x9E3779B1u + s_hx[k]) ^ ((unsigned int)bcy * 0x85EBCA77u + s_hy[k]);
                    h ^= h >> 15;
                    const unsigned int node = (indexed && s_valid[k]) ? 1u + (unsigned int)(qtype - 1) * (bg.hmask + 1u) + (h & bg.hmask) : 0u;
                    id[k] = 0x7fffffff; la[k] = 0x7fffffff; nx[k] = 0; ny[k] = 0;
                    if (node) {
                        const QS_GLOBAL char *const row = (const QS_GLOBAL char *)g_nodes + (node * (unsigned int)sizeof(QsLmNode) + s_se8[k]);
                        id[k] = *(const QS_GLOBAL int *)row;
                        nx[k] = *(const QS_GLOBAL double *)(row + offsetof(QsLmNode, x));
                        ny[k] = *(const QS_GLOBAL double *)(row + offsetof(QsLmNode, y));
                        if (s_last[k]) {
                            // what the owner's `more` asks of a bucket's last entry, in one word: the look-ahead word, or "none" without a successor
                            const int lw = *(const QS_GLOBAL int *)((const QS_GLOBAL char *)g_nodes + (node * (unsigned int)sizeof(QsLmNode) + la_off));
                            la[k] = g_next[node] != 0 ? lw : 0x7fffffff;
                        }
                    }
                }
                const long long lim = (long long)rec.node - mb1, eff = fr < lim ? fr : lim;
                const int eff32 = eff < 0 ? -1 : (int)eff;                          // (limit < 0x7f7f7f7f)
                const unsigned int p = w & 1u;
#pragma unroll
                for (int k = 0; k < FR_SC_KW; k++) {
                    sg_idla[o][p][s_slot[k]] = (long long)(((unsigned long long)(unsigned int)la[k] << 32) | (unsigned int)id[k]);
                    sg_x[o][p][s_slot[k]] = nx[k]; sg_y[o][p][s_slot[k]] = ny[k];
                }
                LDS_CBAR();
                if (lane == 0) {
                    sg_tag[o][p][sc_q] = (indexed && nm == 0) ? c2 : ~0u;            // (a side list or a type beyond the directory: the owner's own query)
                    sg_bcx[o][p][sc_q] = bcx; sg_bcy[o][p][sc_q] = bcy; sg_eff[o][p][sc_q] = eff32;
                    if (sc_q == 0) {
                        sg_rnode[o][p] = rec.node; sg_rr[o][p] = rec.r; sg_rskip[o][p] = rec.skip; sg_rtype[o][p] = rec.type;
                        sg_rpx[o][p] = rec.px; sg_rpy[o][p] = rec.py;
                    }
                }
                LDS_CBAR();
                if (lane == 0) LDS_ST_RLX(&sg_ready[o][p][sc_q], w);
                ah_c2 = pv_skip < j_last ? pv_skip : j_last;
                ah = plan_rec(pl + ah_c2);
            }
        }
