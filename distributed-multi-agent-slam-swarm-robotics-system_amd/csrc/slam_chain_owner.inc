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
            int rid32 = 0x7fffffff;
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
                rid32 = 0x7fffffff; rows.nx = 0; rows.ny = 0; rows.nxt = 0;
                if (node0) {
                    const QS_GLOBAL char *const row = (const QS_GLOBAL char *)g_nodes + (node0 * (unsigned int)sizeof(QsLmNode) + l_se8);
                    rid32 = *(const QS_GLOBAL int *)row;
                    rows.nx = *(const QS_GLOBAL double *)(row + offsetof(QsLmNode, x));
                    rows.ny = *(const QS_GLOBAL double *)(row + offsetof(QsLmNode, y));
                    rows.nxt = g_next[node0];
                }
            };
            if (elig) { if constexpr (LEAN) start_decision_lean(elig); else start_decision(elig); }
            while (elig) {
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
                // full within the limit, has a successor, and ends below the match (a bucket with a hit of its own ends at or
                // above the match, so "has no hit" needs no term).  A match and no such bucket: decided -- free_query would
                // leave its loop after this round with the same match, and with an empty side list return it.  Anything else:
                // free_query, from the same rows, as if nothing had been looked at.
                bool fast = false;
                if constexpr (LEAN) {
                    if (nm_rows == 0) {
                        const long long eff = fr_rows < limit ? fr_rows : limit;
                        const int eff32 = __builtin_amdgcn_readfirstlane(eff < 0 ? -1 : (int)eff);   // (limit < 0x7f7f7f7f)
                        const bool inlim = rid32 <= eff32;
                        const double dx = qx_c - rows.nx, dy = qy_c - rows.ny;
                        const bool hit = inlim && dx * dx + dy * dy < r2thr;                  // :308-309
                        if (__ballot(hit)) {
                            const unsigned int g32 = wave_min_u32(hit ? (unsigned int)rid32 : 0xffffffffu);
                            const unsigned long long more = __ballot(inlim) & ~__ballot(rid32 >= (int)g32) & __ballot(rows.nxt != 0) & L_LAST9;
                            if (more == 0) {
                                const int w = __ffsll((long long)__ballot(hit && rid32 == (int)g32)) - 1;
                                gbest = (long long)g32; wx = rlf64(rows.nx, w); wy = rlf64(rows.ny, w);
                                fast = true;
                            } else if (!DENSE) {
                                // A match, and buckets to walk further: free_query's loop from its second round on, on the low
                                // words -- a lane keeps its first hit, a bucket goes on while it has no hit, its node is full
                                // within the limit and ends below the best match so far, and has a successor.  (DENSE counts
                                // rounds towards its scan of the log: it takes the general query from the start.)
                                st_slow++;
                                const int l_last = min(l_nbk * QS_NODE_CAP + QS_NODE_CAP - 1, 63);
                                unsigned int node = ((more >> l_last) & 1ull) ? rows.nxt : 0u, g = g32;
                                int best32 = hit ? rid32 : 0x7fffffff;
                                double bx = rows.nx, by = rows.ny;
                                while (__ballot(node != 0)) {
                                    int id = 0x7fffffff; double nx = 0, ny = 0; unsigned int nxt = 0;
                                    if (node) {
                                        const QS_GLOBAL char *const row = (const QS_GLOBAL char *)g_nodes + (node * (unsigned int)sizeof(QsLmNode) + l_se8);
                                        id = *(const QS_GLOBAL int *)row;
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
                                    const unsigned long long goon = __ballot(inl) & ~__ballot(id >= (int)g);
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
