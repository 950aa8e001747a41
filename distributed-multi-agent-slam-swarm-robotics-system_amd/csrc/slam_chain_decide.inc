// One decision of an owner wave of qs_slam_chain_free_kernel (slam.hip), from the rows asked for at its start to its match
// (gbest, wx, wy; LL_MAX: none): included by the owner's loop over its chunks (slam_chain_owner.inc) and by the lean owner's
// walk of its plan (slam_chain_plan_owner.inc).  Everything it names is theirs or the kernel's.
                const long long qidx_c = qidx;                                      // (this decision's: start_decision below moves on)
                const double qx_c = qx, qy_c = qy;
                const int f_c = f, qtype_c = qtype;
                // :300 -- and a node never sees its own landmark (appended after the check, :288): with MIN_POSES_BETWEEN < 1
                // the newest landmark a query can see is still the one before it
                const long long limit = qidx_c - (min_between > 1 ? min_between : 1);
                long long gbest = LL_MAX; double wx = 0, wy = 0;
                // The lean owner's decision by the first rows alone -- what free_query's first round works out, on 32-bit indices:
                // who is within the limit (eff = min(frontier as read before the rows, limit); negative: nobody) and within the
                // radius, the lowest index among them, and whether any bucket would have to be walked further: one whose node is
                // full within the limit, has a successor, and whose successor starts below the match.  A match and no such
                // bucket: decided -- free_query would find nothing lower behind it, and with an empty side list return the same
                // match.  Anything else: free_query, from the same rows, as if nothing had been looked at.
                // "Starts below the match" is read from the node's look-ahead word (rla32: QsLmNode, qs_internal.h), and is exact:
                // a chain's entries are in insertion order, so all of a successor chain lies at or above its first entry, and a
                // chain whose first entry is not below the match cannot lower the minimum.  An empty word reads 0x7f7f7f7f, above
                // every index and every eff: nothing to go on to.  It cannot read empty while a successor entry at or below eff
                // exists: that entry's batch, the look-ahead store included, was complete before the frontier that was read
                // ahead of the loads.  (With the look-ahead switched off -- la_off, qs_set_chain_lookahead -- the same load
                // brings the node's last entry: "ends below the match", free_query's rule; a bucket with a hit of its own ends
                // at or above the match, so "has no hit" needs no term.)
                bool fast = false;
                if constexpr (LEAN) {
                    if (nm_rows == 0) {
                        const int eff32 = lean_eff32(limit);
                        const bool inlim = rid32 <= eff32;
                        const double dx = qx_c - rows.nx, dy = qy_c - rows.ny;
                        const bool hit = inlim && dx * dx + dy * dy < r2thr;                  // :308-309
                        if (__ballot(hit)) {
                            const unsigned int g32 = wave_min_u32(hit ? (unsigned int)rid32 : 0xffffffffu);
                            const unsigned long long more = __ballot(inlim) & ~__ballot(rla32 >= (int)g32) & __ballot(rows.nxt != 0) & L_LAST9;
                            if (more == 0) {
                                const int w = __ffsll((long long)__ballot(hit && rid32 == (int)g32)) - 1;
                                gbest = (long long)g32; wx = rlf64(rows.nx, w); wy = rlf64(rows.ny, w);
                                fast = true;
                            } else if (!DENSE) {
                                // A match, and buckets to walk further: free_query's loop from its second round on, on the low
                                // words -- a lane keeps its first hit, a bucket goes on while it has no hit, its node is full
                                // within the limit, has a successor, and that successor starts below the best match so far (the
                                // round's node's look-ahead word, as above).  (DENSE counts rounds towards its scan of the log:
                                // it takes the general query from the start.)
                                st_slow++;
                                const int l_last = min(l_nbk * QS_NODE_CAP + QS_NODE_CAP - 1, 63);
                                unsigned int node = ((more >> l_last) & 1ull) ? rows.nxt : 0u, g = g32;
                                int best32 = hit ? rid32 : 0x7fffffff;
                                double bx = rows.nx, by = rows.ny;
                                while (__ballot(node != 0)) {
                                    int id = 0x7fffffff, la = 0x7fffffff; double nx = 0, ny = 0; unsigned int nxt = 0;
                                    if (node) {
                                        const QS_GLOBAL char *const row = (const QS_GLOBAL char *)g_nodes + (node * (unsigned int)sizeof(QsLmNode) + l_se8);
                                        id = *(const QS_GLOBAL int *)row;
                                        la = *(const QS_GLOBAL int *)((const QS_GLOBAL char *)g_nodes + (node * (unsigned int)sizeof(QsLmNode) + la_off));
                                        nx = *(const QS_GLOBAL double *)(row + offsetof(QsLmNode, x));
                                        ny = *(const QS_GLOBAL double *)(row + offsetof(QsLmNode, y));
                                        nxt = g_next[node];
                                    }
                                    const bool inl = id <= eff32;
                                    bool newhit = false;
                                    if (inl && best32 == 0x7fffffff) {
                                        const double ex = qx_c - nx, ey = qy_c - ny;
                                        if (ex * ex + ey * ey < r2thr) { best32 = id; bx = nx; by = ny; newhit = true; }   // :308-309
                                    }
                                    if (__ballot(newhit)) { const unsigned int v = wave_min_u32(newhit ? (unsigned int)id : 0xffffffffu); g = v < g ? v : g; }
                                    const unsigned long long hitm = __ballot(best32 != 0x7fffffff);
                                    const unsigned long long goon = __ballot(inl) & ~__ballot(la >= (int)g);
                                    const bool b_hit = ((hitm >> (l_nbk * QS_NODE_CAP)) & 0x7full) != 0;
                                    if (node) node = (b_hit || !((goon >> l_last) & 1ull) || nxt == 0) ? 0u : nxt;
                                }
                                const int w = __ffsll((long long)__ballot(best32 == (int)g)) - 1;
                                gbest = (long long)g; wx = rlf64(bx, w); wy = rlf64(by, w);
                                fast = true;
                            }
                        }
                    }
                    if (!fast) {                                                            // the rows as free_query takes them
                        st_slow++;
                        rows.id = rid32 >= 0x7f7f7f7f ? LL_MAX : (long long)rid32;
                        const int last32 = __shfl(rid32, min(l_nbk * QS_NODE_CAP + QS_NODE_CAP - 1, 63));
                        rows.lastid = last32 >= 0x7f7f7f7f ? LL_MAX : (long long)last32;
                    }
                }
                if (!fast) {
                    bool pre = true;
                    for (long long fr = fr_rows;;) {
                        const long long nm = s_nmisc, nl = DENSE ? s_nlms : 0;
                        gbest = free_query<DENSE>(Gp, g_nodes, g_next, bg, qx_c, qy_c, qtype_c, fr < limit ? fr : limit, r2thr, nm, nl, lane, wx, wy, st_misc,
                                                  node0, pre, rows);
                        if (gbest != LL_MAX || fr >= limit) break;                  // a match below the frontier is final; so is "none" once all are in
                        pre = false;
                        // Nothing in the index up to fr.  The landmarks with fr < node <= limit are events the committer has not got
                        // to: their poses are in the pending ring once their owners have passed them.  64 events a round, youngest
                        // first; the OLDEST match is the reference's first match.
                        st_wait++;
                        publish_prog(qidx_c);                                       // (the committer has to get past this owner's older events)
                        if (!POST) {                                                // wait until it has everything up to the limit in the index
                            if (lds_ld64(&s_frontier) <= fr) FR_SPIN(lds_ld64(&s_frontier) < limit);
                            fr = lds_ld64(&s_frontier);
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");    // the index as of that frontier, not older
                            continue;
                        }
                        bool stale = false;
                        const unsigned int r_me = q0 - e0 + (unsigned int)f_c;      // this event's place in the list
                        for (unsigned int back = 0; back < r_me; back += QS_WAVE) {
                            const long long jr = (long long)r_me - 1 - (long long)back - lane;
                            const bool hv = jr >= 0;
                            const long long nd = hv ? sb.ev_node[e0 + (unsigned int)jr] : -LL_MAX - 1;
                            const int ty = hv ? (int)sb.ev_type[e0 + (unsigned int)jr] : 0;
                            const bool inr = hv && nd > fr && nd <= limit;
                            const unsigned int ps = hv ? (unsigned int)jr % FR_PEND : 0u;
                            // posted -- or, if the committer overtook it meanwhile (its slot may have a new holder), in the index by now
                            FR_SPIN(__ballot(inr && LDS_RLX(&p_node[ps]) != nd && LDS_RLX(&s_frontier) < nd) != 0);
                            LDS_CBAR();
                            if (__ballot(inr && LDS_RLX(&p_node[ps]) != nd)) { stale = true; break; }
                            bool hit = false;
                            double lx = 0, ly = 0;
                            if (inr && ty == qtype_c) {
                                lx = p_x[ps]; ly = p_y[ps];
                                const double dx = qx_c - lx, dy = qy_c - ly;
                                hit = dx * dx + dy * dy < r2thr;                    // :308-309
                            }
                            LDS_CBAR();
                            if (__ballot(inr && LDS_RLX(&p_node[ps]) != nd)) { stale = true; break; }
                            const unsigned long long hm = __ballot(hit);
                            if (hm) { const int w = 63 - __builtin_clzll(hm); gbest = rl64(nd, w); wx = rlf64(lx, w); wy = rlf64(ly, w); }
                            if (!__ballot(hv && lane == QS_WAVE - 1 && nd > fr)) break;  // the round's oldest event is in the index already
                        }
                        if (!stale) break;                                          // match or none: final (index up to fr, events up to limit)
                        gbest = LL_MAX;                                             // the index has grown under the scan: once more, from it
                        fr = lds_ld64(&s_frontier);
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");        // the index as of that frontier, not older
                    }
                }
