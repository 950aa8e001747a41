"""Live UDP front-end: the reference's main() loop without the renderer.

Mirrors server_nodes/dual_bot_mapper.py:
  socket            :745-753   UDP, SO_REUSEADDR, bind 0.0.0.0:port, non-blocking
  receive           :815-848   drain datagrams, remember each bot's source IP, reply port 8888 for
                               bot 1 / 8889 for bot 2 (:759, :846), per-bot packet counts
  per-packet body   :826-919   handed to the GPU as ONE batch per poll (QuasarMapper.ingest_array)
  heartbeat         :805-812   5 s of silence -> offline; any accepted packet -> online (:860-864)
  zone timer        :922-945   every > 2 s: each bot gets the OTHER bot's bounding box, or the lift
                               box (999, 999, -999, -999) when the other is offline
  target timer      :947-996   every > 3 s: the online bots, ascending id, are given the nearest frontier
                               centroid not taken and not within FRONTIER_SEPARATION of an earlier target, sent
                               as TARG (:691-699).  Commented out in the reference as shipped, so opt-in here
                               (frontier_targets=True); the mapper then also needs assign_frontier_targets.
                               With plan_paths=True (also opt-in) a TARG carries instead the waypoint of a path over
                               the mapped free space to that centroid (QuasarMapper.plan_paths), or the centroid itself
                               when there is no path; plan_params go to plan_paths.
                               With targets_by_path=True (also opt-in) the centroids are ranked by path cost instead
                               of straight-line distance (QuasarMapper.assign_frontier_targets(by_path=True), ONE
                               device call per tick, plan_params its planning parameters): every assigned bot has a
                               path to its target, so with plan_paths=True every TARG carries a waypoint.
                               With targets_by_territory=True (also opt-in, excludes targets_by_path) the mapped free
                               space is partitioned among the online bots by path cost and each bot takes the cheapest
                               centroid of its own share (QuasarMapper.assign_frontier_targets(by_territory=True), ONE
                               device call per tick); with plan_paths=True every TARG carries a waypoint.  `territory`
                               then holds {bot: (cells owned, world box or None)} of the last tick.
                               With targets_by_gain=True (also opt-in, excludes the other two) the centroids are ranked by
                               the unknown area a bot would see from them over the path cost
                               (QuasarMapper.assign_frontier_targets(by_gain=True), ONE device call per tick; gain_params:
                               gain_range, gain_bias); TARG and plan_stats as with targets_by_path.
Servo sweeps (opt-in, sweeps=True): the 743-byte v0 and 751-byte v0 + odometry packets of the ESP32 firmware
(esp32_firmware/src/main.cpp:190-215) are mapped too.  Datagrams then get slots of SWEEP_SLOT bytes; the datagrams of a
poll are cut, in arrival order, into maximal runs of one kind (41/42-byte packets, 743-byte sweeps, 751-byte sweeps),
each run one ingest call.  No call names its sequence numbers: the mapper continues its own counter across both kinds
(1 per packet, 46 per sweep), so stamps follow arrival, after whatever the mapper held before (a replayed log, say).  An accepted sweep marks its bot online and sets its pose, as a packet does.
With match_sweeps=True (opt-in, needs sweeps=True) a run of sweeps is matched against the map before it is mapped
(QuasarMapper.ingest_sweeps(match=...), match_params its parameters): the bot's pose is then the corrected one, and
last_matches holds the matches of the latest run.
With sweep_graph=True or a dict of half_width / close / open (opt-in, needs sweeps=True) the mapper is put into graph mode at
construction (QuasarMapper.set_sweep_graph): sweeps become pose-graph nodes, close loops and feed their bot's zone box, so
zone_tick sends a sweep bot's partner a real box.
With relocalise=True or a dict of relocalisation parameters (opt-in, needs sweeps=True, excludes sweep_graph: drift would move
under the transform) the first accepted sweep of a bot that was offline, or was never seen, is located against the whole map
before it is mapped (QuasarMapper.relocalise_sweeps).  When the gate accepts, the front-end keeps a rigid transform for that bot,
from the pose the ingest would have formed (the packet's pose plus QuasarMapper.sweep_pose_shift) to the found pose, and
rewrites the f32 x / y / yaw fields of that bot's sweep records from then on, the triggering one included, in its own buffer
before they are ingested.  relocalised[bot] holds the latest accepted result, reloc_stats counts tried / accepted / rewritten.
A relocalisation the gate does not accept changes nothing.
With relocalise={"group": K, "travel": m, ...} (K in 2..RELOC_MAX_GROUP; travel defaults to RELOC_TRAVEL) a bot that comes online
without a transform is located from several sweeps scored jointly (QuasarMapper.relocalise_groups): copies of its accepted sweeps
are kept, up to K, those whose pose lies within `travel` of the first kept one; after each run that adds one the kept records are
relocalised as one group whose frame is the first kept record.  On acceptance the transform is set from that record's ingest
pose, as above, and the copies are dropped; after K records without acceptance the front-end gives up on that bot until it is
next found offline.  Sweeps are ingested meanwhile as they arrive.  reloc_stats then also counts group_tried / gave_up.
With check_sweeps=True or a dict of check parameters plus lost_after (opt-in, needs sweeps=True, excludes sweep_graph and
match_sweeps) a run of sweeps goes through the guarded ingest (QuasarMapper.ingest_sweeps(check=...)): a sweep that contradicts
the map is withheld from it.  last_checks holds the checks of the latest run, check_stats counts checked / withheld / undecided,
suspect[bot] is the bot's run of consecutive contradicted sweeps (an OK sweep resets it, an undecided one leaves it).  A withheld
sweep still counts for the heartbeat; it does not move the bot's pose.  With relocalise also on, a bot whose run reaches
lost_after (default CHECK_LOST_AFTER) loses its transform and is relocalised from its next sweep on exactly as a bot found
offline is, group mode included, until a relocalisation is accepted.
With match_packets=True or a dict (opt-in; works with and without sweeps=True) the 42-byte packets are matched against the map
as TRAILS before they are mapped (QuasarMapper.match_trails; include/quasar_slam.h, "trail matching").  A trail matched after its
own packets are in the map agrees with its own hits at zero displacement, so the front-end holds packets back: a packet datagram
that passes the host-side pre-check (length 42 / 41, magic, agent range) is copied to its bot's pending list instead of being
ingested; it still shows that its bot is there (address, heartbeat).  Every other datagram goes to the ingest at once.  After a
poll's runs a bot flushes when its list holds `trail` records (default and at most TRAIL_MAX_RECORDS) or its oldest is `hold`
seconds old (default 5.0): the flushing bots' records, rewritten by their transforms in force, are matched in ONE match_trails
call, one group per bot (`travel`, default TRAIL_TRAVEL; every other key of the dict is a match parameter).  An accepted match
with a non-zero candidate is composed into that bot's rigid transform (rule T7, formed with QuasarMapper.sweep_pose_shift at
match time; a later closure's drift is not turned with it), which rewrites the f32 x / y / yaw fields of the bot's packets from
then on, the trail's own included.  Then all flushed records go, in arrival order, through ONE ingest_array, as a poll's packets
do.  flush_trails() flushes everything pending (close() calls it); trail_matches[bot] holds the bot's latest result, trail_stats
counts held / tried / accepted / moved / rewritten.  A bot that delivers more than `trail` packets to one poll flushes in rounds.
With match_packets={"relocalise": True or a dict of relocalisation parameters, "tries": 4, "bots": [...], ...} (opt-in inside the
opt-in) a packet bot whose frame is unknown is first FOUND (QuasarMapper.relocalise_trails; include/quasar_slam.h, "trail
relocalisation"): a bot that comes online, the first time or back from offline, without a transform -- any bot but the first one
ever seen, whose frame is the map's, or those named in "bots" -- has its due trails located over the whole map instead of matched,
and held instead of mapped.  On acceptance the found frame (rule K7, less sweep_pose_shift) becomes the bot's transform, all it
held is rewritten by it and mapped in arrival order, and its later trails are matched as above; after "tries" refusals (or at
flush_trails()) what it held is mapped as it is and the bot is left alone until it is next found offline.  trail_stats then
also counts reloc_tried / reloc_accepted / reloc_gave_up; trail_relocs[bot] holds the latest result.
With track_view=True (opt-in) the front-end keeps what the reference's renderer is handed each frame (:878-892):
point_clouds[bot][sensor], the hit points of the accepted packets (QuasarMapper.last_hits), and paths[bot] = ([xs], [ys]), their
poses; mapper.MapView.frame draws them.
Differences: the reference throttles itself to 20 packets per 30 fps frame (:816, :474); here a
poll drains the socket (up to max_batch datagrams).  Host-side Python only; the mapper can be any
object with ingest_array / last_batch / zone_packet (tests use a stub, production the HIP mapper).
"""
import socket
import time

import numpy as np

from . import protocol as P

SLOT = 48      # bytes per datagram slot handed to qs_ingest (42-byte packets, room for oversize marks)
SWEEP_SLOT = 752   # with sweeps on: room for a 751-byte sweep and the oversize mark


class MissionControl:
    def __init__(self, mapper, port=8888, bind_addr="0.0.0.0", max_batch=65536, sock=None, max_agent=2,
                 frontier_targets=False, sweeps=False, plan_paths=False, plan_params=None, match_sweeps=False,
                 match_params=None, targets_by_path=False, sweep_graph=False, track_view=False,
                 targets_by_territory=False, targets_by_gain=False, gain_params=None, relocalise=False, check_sweeps=False,
                 match_packets=False, bot_veil=False):
        by = [k for k, on in (("targets_by_path", targets_by_path), ("targets_by_territory", targets_by_territory),
                              ("targets_by_gain", targets_by_gain)) if on]
        if not frontier_targets and (plan_paths or by):         # each of them refines frontier_targets
            raise ValueError(f"MissionControl: {by[0] if by else 'plan_paths'}=True needs frontier_targets=True")
        if len(by) > 1:                                         # and at most one ranking is in force
            raise ValueError(f"MissionControl: {by[-1]}=True excludes {' and '.join(by[:-1])}")
        if match_sweeps and not sweeps:
            raise ValueError("MissionControl: match_sweeps=True needs sweeps=True")
        self.sweep_graph = sweep_graph is not False and sweep_graph is not None      # ({} is on, with the defaults)
        if self.sweep_graph and not sweeps:
            raise ValueError("MissionControl: sweep_graph needs sweeps=True")
        self.relocalise = relocalise is not False and relocalise is not None          # ({} is on, with the defaults)
        if self.relocalise and not sweeps:
            raise ValueError("MissionControl: relocalise needs sweeps=True")
        if self.relocalise and self.sweep_graph:
            raise ValueError("MissionControl: relocalise excludes sweep_graph (a closure's drift would move under the transform)")
        self.check_sweeps = check_sweeps is not False and check_sweeps is not None      # ({} is on, with the defaults)
        if self.check_sweeps and not sweeps:
            raise ValueError("MissionControl: check_sweeps needs sweeps=True")
        if self.check_sweeps and self.sweep_graph:
            raise ValueError("MissionControl: check_sweeps excludes sweep_graph (a withheld sweep would still be a node)")
        if self.check_sweeps and match_sweeps:
            raise ValueError("MissionControl: check_sweeps excludes match_sweeps (the guarded and the matched ingest do not combine)")
        self.check_params = dict(check_sweeps) if isinstance(check_sweeps, dict) else True
        self.lost_after = int(self.check_params.pop("lost_after")) if self.check_params is not True and "lost_after" in self.check_params \
            else P.CHECK_LOST_AFTER
        if self.lost_after < 1:
            raise ValueError("MissionControl: check_sweeps['lost_after'] must be at least 1")
        if self.sweep_graph:
            mapper.set_sweep_graph(True, **(dict(sweep_graph) if isinstance(sweep_graph, dict) else {}))
        self.reloc_params = dict(relocalise) if isinstance(relocalise, dict) else True
        self.reloc_group = self.reloc_travel = None
        if isinstance(relocalise, dict) and "group" in relocalise:
            self.reloc_group = int(self.reloc_params.pop("group"))
            self.reloc_travel = float(self.reloc_params.pop("travel", P.RELOC_TRAVEL))
            if not 2 <= self.reloc_group <= P.RELOC_MAX_GROUP:
                raise ValueError("MissionControl: relocalise['group'] must lie in [2, RELOC_MAX_GROUP]")
        elif isinstance(relocalise, dict) and "travel" in relocalise:
            raise ValueError("MissionControl: relocalise['travel'] needs 'group'")
        self._reloc_kept = {}                        # bot -> copies of its kept sweeps (group mode, while it is being located)
        self.relocalised = {}                        # bot -> the accepted result (a record of protocol.RELOC_DTYPE) in force
        self.reloc_stats = {"tried": 0, "accepted": 0, "rewritten": 0}
        if self.reloc_group:
            self.reloc_stats.update(group_tried=0, gave_up=0)
        self._reloc_T = {}                           # bot -> (cos, sin, dyaw, ingest x, y, found x, y, shift x, y)
        self.check_stats = {"checked": 0, "withheld": 0, "undecided": 0}
        self.suspect = {b: 0 for b in range(1, max_agent + 1)}     # bot -> its run of consecutive contradicted sweeps
        self._lost = set()                           # bots whose run reached lost_after: relocalised as a bot found offline is
        self.last_checks = None
        self.match_packets = match_packets is not False and match_packets is not None      # ({} is on, with the defaults)
        self.trail_params = dict(match_packets) if isinstance(match_packets, dict) else {}
        self.trail = int(self.trail_params.pop("trail", P.TRAIL_MAX_RECORDS))
        self.trail_hold = float(self.trail_params.pop("hold", 5.0))
        self.trail_travel = float(self.trail_params.pop("travel", P.TRAIL_TRAVEL))
        # "relocalise": True or a dict of relocalisation parameters: bots that come online without a transform are first LOCATED
        # over the whole map from their trails (QuasarMapper.relocalise_trails), at most "tries" trails each
        reloc = self.trail_params.pop("relocalise", None)
        self.trail_reloc = reloc is not None and reloc is not False
        self.trail_reloc_params = dict(reloc) if isinstance(reloc, dict) else None
        self.trail_reloc_tries = int(self.trail_params.pop("tries", 4)) if self.trail_reloc else 0
        bots_ = self.trail_params.pop("bots", None) if self.trail_reloc else None
        self.trail_reloc_bots = None if bots_ is None else {int(b) for b in bots_}
        self._first_bot = None                       # the first bot ever seen: its frame is the map's, it is never located
        self._locating = {}                          # bot -> [trails tried, its held packets]: not mapped until found or given up
        self.trail_relocs = {}                       # bot -> its latest result (a record of protocol.TRAIL_RELOC_DTYPE)
        if not 1 <= self.trail <= P.TRAIL_MAX_RECORDS:
            raise ValueError("MissionControl: match_packets['trail'] must lie in [1, TRAIL_MAX_RECORDS]")
        self._pending = {b: [] for b in range(1, max_agent + 1)}   # bot -> held packets (arrival number, record, length, time, address)
        self._trail_seq = 0
        self._trail_T = {}                           # bot -> (cos, sin, angle, tx, ty): field (x, y) -> R (x, y) + t, yaw + angle
        self.trail_matches = {}                      # bot -> its latest result (a record of protocol.TRAIL_MATCH_DTYPE)
        self.trail_stats = {"held": 0, "tried": 0, "accepted": 0, "moved": 0, "rewritten": 0}
        if self.trail_reloc:
            self.trail_stats.update(reloc_tried=0, reloc_accepted=0, reloc_gave_up=0)
        # bot_veil=True or {"radius": r}: the mapper's bot veil (QuasarMapper.set_bot_veil) is turned on here; a bot found offline
        # is forgotten (carried away, it must not leave a blind disc), and with sweeps=True every sweep bot is placed at the pose
        # of its latest accepted sweep after each sweep ingest (sweep ingests do not feed the veil's table themselves) -- unless
        # bot_veil={"radius": r, "sweeps": True} turns the mapper's sweep switch on: then the device veils sweep beams and feeds the
        # table from the sweeps itself, and nothing is placed here
        self.bot_veil = bot_veil is not False and bot_veil is not None
        self.bot_veil_sweeps = isinstance(bot_veil, dict) and bool(bot_veil.get("sweeps"))
        if self.bot_veil:
            mapper.set_bot_veil(**(dict(bot_veil) if isinstance(bot_veil, dict) else {}))
        self.track_view = track_view
        self.point_clouds = {b: {s: [] for s in P.SENSOR_NAMES} for b in range(1, max_agent + 1)}      # :768-771
        self.paths = {b: ([], []) for b in range(1, max_agent + 1)}                                    # :772
        self.match_sweeps = match_sweeps
        self.match_params = dict(match_params) if match_params else True
        self.last_matches = None
        self.mapper = mapper
        self.plan_paths = plan_paths
        self.targets_by_path = targets_by_path
        self.targets_by_territory = targets_by_territory
        self.targets_by_gain = targets_by_gain
        self.gain_params = dict(gain_params or {})
        self.territory = {}
        self.plan_params = dict(plan_params or {})
        self.plan_stats = {"waypoint": 0, "centroid": 0}
        self.sweeps = sweeps
        self.slot = SWEEP_SLOT if sweeps else SLOT
        self.frontier_targets = frontier_targets
        self.max_agent = max_agent
        self.max_batch = max_batch
        if sock is None:
            sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)                   # :745
            sock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)                # :746
            sock.bind((bind_addr, port))                                              # :748
        sock.setblocking(False)                                                       # :753
        self.sock = sock
        bots = range(1, max_agent + 1)
        self.bot_addrs = {b: None for b in bots}                                      # :758
        self.bot_ports = {b: 8887 + b for b in bots}                                  # :759  (1 -> 8888, 2 -> 8889)
        self.last_packet_time = {b: 0.0 for b in bots}                                # :760
        self.pkt_counts = {b: 0 for b in bots}                                        # :761
        self.online = {b: False for b in bots}
        self.seen = {b: False for b in bots}
        self.zone_boxes = {b: None for b in bots}                                     # :773
        self.last_zone_send = time.time()                                             # :788
        self.bot_pose = {b: None for b in bots}      # bot_states[b]['x'], ['y']: last accepted pose (:850-866)
        self.last_target_send = time.time()
        self._buf = np.zeros((max_batch, self.slot), dtype=np.uint8)
        self._lens = np.zeros(max_batch, dtype=np.uint16)
        self._times = np.zeros(max_batch, dtype=np.float64)
        self._addrs = [None] * max_batch
        self.datagrams = 0

    # ---- :815-848 + :826-919 -----------------------------------------------------------------
    def poll(self, now=None):
        """Drain the socket into one batch and ingest it.  Returns the number of datagrams."""
        now = time.time() if now is None else now
        n = 0
        SL = self.slot
        view = memoryview(self._buf).cast("B")
        while n < self.max_batch:
            try:
                nbytes, addr = self.sock.recvfrom_into(view[n * SL:(n + 1) * SL], SL)   # :818
            except BlockingIOError:
                break
            except OSError:
                break
            self._lens[n] = nbytes if nbytes < SL else 65535       # a datagram that fills the slot may be longer: drop it
            self._times[n] = now
            self._addrs[n] = addr
            n += 1
        if not self.match_packets:
            if n:
                self.datagrams += n
                self._ingest_runs(n, now)
            return n
        self.datagrams += n
        rest = self._hold(n, now) if n else 0
        if rest:
            self._ingest_runs(rest, now)
        self._flush_trails(now, False)
        return n

    def _ingest_runs(self, n, now):
        """The first n slots of the receive buffer through the mapper: one ingest, or (sweeps) one per run of a kind."""
        if not self.sweeps:
            self._ingest_packets(0, n, now)
            return
        for i0, i1, kind in self._runs(n):
            lens = self._lens[i0:i1]
            if kind == 0:
                self._ingest_packets(i0, i1, now)
            else:
                if self.relocalise:
                    self._relocalise_run(self._buf[i0:i1, :kind], lens)
                if self.match_sweeps:
                    self.mapper.ingest_sweeps(self._buf[i0:i1, :kind], lens, match=self.match_params)
                    self.last_matches = self.mapper.last_sweep_matches()
                elif self.check_sweeps:
                    self.mapper.ingest_sweeps(self._buf[i0:i1, :kind], lens, check=self.check_params)
                    self.last_checks = self.mapper.last_sweep_checks()
                else:
                    self.mapper.ingest_sweeps(self._buf[i0:i1, :kind], lens)
                accepted, pose = self.mapper.last_sweeps()
                self._mark(i0, accepted, pose, now, pose is not None)
                if self.check_sweeps:
                    self._note_checks(i0, self.last_checks, now)
                if self.bot_veil and not self.bot_veil_sweeps and pose is not None:
                    latest = {int(self._buf[i0 + int(j), 4]): int(j) for j in np.nonzero(accepted)[0]}
                    for a, j in latest.items():
                        self.mapper.bot_veil_place(a, float(pose[j, 0]), float(pose[j, 1]))

    def _ingest_packets(self, i0, i1, now, held=None):
        """Slots i0 .. i1 of the receive buffer as one packet ingest, and its bookkeeping.  held (match_packets): the flushed
        records (buf, lens, times, addrs) in their place; they showed at arrival that their bots are there, so mapping them now
        does not count for the heartbeat."""
        buf, lens, times, addrs = held if held is not None else (self._buf, self._lens, self._times, self._addrs)
        self.mapper.ingest_array(buf[i0:i1, :SLOT], lens[i0:i1], times[i0:i1])
        accepted, pose = self.mapper.last_batch()
        self._mark(i0, accepted, pose, now, self.frontier_targets and pose is not None, buf, addrs, heartbeat=held is None)
        if self.track_view:
            self._track(i0, accepted, pose, buf)

    # ---- match_packets: packets held back, matched as trails, then mapped ----------------------------------------------------
    def _hold(self, n, now):
        """The packet datagrams among the first n slots that pass the pre-check move to their bots' pending lists; the other
        datagrams close ranks in the receive buffer.  Returns how many those are."""
        buf, lens = self._buf[:n], self._lens[:n]
        ok = (((lens == P.PACKET_SIZE) | (lens == P.PACKET_SIZE_V1)) & (buf[:, :4] == np.frombuffer(b"QSRL", dtype=np.uint8)).all(axis=1)
              & (buf[:, 4] >= 1) & (buf[:, 4] <= self.max_agent))
        held = np.nonzero(ok)[0]
        if len(held) == 0:
            return n
        for i in held:
            a = int(buf[i, 4])
            self._pending[a].append((self._trail_seq, buf[i, :SLOT].copy(), int(lens[i]), float(self._times[i]), self._addrs[i]))
            self._trail_seq += 1
            if self.trail_reloc:
                self._note_arrival(a)
            self.bot_addrs[a] = (self._addrs[i][0], self.bot_ports[a])      # the bot is there, as a withheld sweep shows it
            self.last_packet_time[a] = now
            self.online[a] = True
            self.seen[a] = True
        self.trail_stats["held"] += len(held)
        rest = np.nonzero(~ok)[0]
        m = len(rest)
        if m:
            self._buf[:m] = self._buf[rest]
            self._lens[:m] = self._lens[rest]
            self._times[:m] = self._times[rest]
            self._addrs[:m] = [self._addrs[i] for i in rest]
        return m

    def _note_arrival(self, bot):
        """match_packets["relocalise"]: a bot that comes online -- the first time, or back from offline -- without a transform is
        due to be located, unless it is the first bot ever seen (whose frame is the map's) or "bots" leaves it out."""
        if self._first_bot is None:
            self._first_bot = next((b for b in sorted(self.seen) if self.seen[b]), bot)
        if self.online[bot] or bot in self._trail_T or bot in self._locating:
            return
        if bot in self.trail_reloc_bots if self.trail_reloc_bots is not None else bot != self._first_bot:
            self._locating[bot] = [0, []]

    def _trail_travel_of(self, recs):
        """The travel a trail needs: the largest distance of a record from the last one, rounded up to the next 0.25 m and capped
        at trail_travel, so that the patch the search stages is no larger than the trail."""
        f = np.ascontiguousarray(recs[:, 5:13]).view("<f4").astype(np.float64)
        d = np.hypot(f[:, 0] - f[-1, 0], f[:, 1] - f[-1, 1])
        d = float(d[np.isfinite(d)].max()) if np.isfinite(d).any() else 0.0
        return min(self.trail_travel, float(np.ceil(d / 0.25)) * 0.25)

    def _trail_locate(self, bot, group, shift):
        """One trail of a bot that is being located.  Returns the packets to map now: none while it is held; on acceptance
        (rule K7's transform, less what the ingest adds itself, becomes the bot's) or after the last try, all it held."""
        tried, held = self._locating[bot]
        recs = np.stack([p[1] for p in group])
        lens = np.array([p[2] for p in group], dtype=np.uint16)
        r = self.mapper.relocalise_trails(recs, [len(group)], lens, travel=self._trail_travel_of(recs),
                                          params=self.trail_reloc_params)[0]
        self.trail_relocs[bot] = r.copy()
        self.trail_stats["reloc_tried"] += 1
        held.extend(group)
        if r["accepted"]:
            self.trail_stats["reloc_accepted"] += 1
            th, ax, ay = float(r["yaw"]), float(r["ax"]), float(r["ay"])
            c, s = np.cos(th), np.sin(th)
            self._trail_T[bot] = (c, s, th, float(r["x"]) - (c * ax - s * ay) - shift[0], float(r["y"]) - (s * ax + c * ay) - shift[1])
        elif tried + 1 < self.trail_reloc_tries:
            self._locating[bot][0] = tried + 1
            return []
        else:
            self.trail_stats["reloc_gave_up"] += 1
        del self._locating[bot]
        return held

    @staticmethod
    def _trail_rewrite(recs, T):
        """The f32 x / y / yaw fields of packet records (uint8 [K, SLOT], in place) moved by the rigid transform T."""
        c, s, th, tx, ty = T
        for rec in recs:
            f = rec[5:17].view("<f4")
            x, y = float(f[0]), float(f[1])
            f[:] = (tx + (c * x - s * y), ty + (s * x + c * y), float(f[2]) + th)

    def _trail_compose(self, bot, r, shift):
        """The correction of match r (rule T7; its anchor in the frame of T3, `shift` = the offset and drift that frame adds to
        the fields) composed onto the bot's transform of the packet fields."""
        sx, sy = shift
        cm, sm = np.cos(float(r["dyaw"])), np.sin(float(r["dyaw"]))
        ax, ay = float(r["ax"]) - sx, float(r["ay"]) - sy             # the anchor in field coordinates
        mx, my = ax + float(r["dx"]) - (cm * ax - sm * ay), ay + float(r["dy"]) - (sm * ax + cm * ay)
        _, _, th, tx, ty = self._trail_T.get(bot, (1.0, 0.0, 0.0, 0.0, 0.0))
        th = th + float(r["dyaw"])
        self._trail_T[bot] = (np.cos(th), np.sin(th), th, (cm * tx - sm * ty) + mx, (sm * tx + cm * ty) + my)

    def _flush_trails(self, now, everything):
        """Flush in rounds, each round one trail per due bot: ONE match_trails call, then ONE ingest of the round's records in
        arrival order.  everything: every bot with a pending packet is due."""
        while True:
            due = {}
            for b, pend in self._pending.items():
                if len(pend) >= self.trail:
                    due[b] = self.trail
                elif pend and (everything or now - pend[0][3] >= self.trail_hold):
                    due[b] = len(pend)
            if not due:
                return
            groups = {}
            for b, k in sorted(due.items()):
                groups[b], self._pending[b] = self._pending[b][:k], self._pending[b][k:]
            shift_of = getattr(self.mapper, "sweep_pose_shift", None)
            located = []                             # what the bots being located release: mapped with this round's records
            for b in [b for b in groups if b in self._locating]:
                located.extend(self._trail_locate(b, groups.pop(b), tuple(float(v) for v in shift_of(b)) if shift_of else (0.0, 0.0)))
            # matched as the transforms in force would map them
            trial = []
            for b, g in groups.items():
                recs = np.stack([p[1] for p in g])
                if b in self._trail_T:
                    self._trail_rewrite(recs, self._trail_T[b])
                trial.append(recs)
            lens = np.array([p[2] for g in groups.values() for p in g], dtype=np.uint16)
            shifts = {b: tuple(float(v) for v in shift_of(b)) if shift_of else (0.0, 0.0) for b in groups}
            res = self.mapper.match_trails(np.concatenate(trial), [len(g) for g in groups.values()], lens,
                                           travel=self.trail_travel, params=self.trail_params or None) if groups else ()
            for b, r in zip(groups, res):
                self.trail_matches[b] = r.copy()
                self.trail_stats["tried"] += 1
                if r["accepted_match"]:
                    self.trail_stats["accepted"] += 1
                    if int(r["ix"]) or int(r["iy"]) or int(r["it"]):
                        self.trail_stats["moved"] += 1
                        self._trail_compose(b, r, shifts[b])
            # mapped, in arrival order, as the transforms now in force map them (the trail's own records included)
            flat = sorted([p for g in groups.values() for p in g] + located, key=lambda p: p[0])
            m = len(flat)
            if m == 0:                               # (every due trail is held by a bot being located)
                continue
            buf = np.zeros((m, self.slot), dtype=np.uint8)
            for j, p in enumerate(flat):
                buf[j, :SLOT] = p[1]
                T = self._trail_T.get(int(p[1][4]))
                if T is not None:
                    self._trail_rewrite(buf[j:j + 1], T)
                    self.trail_stats["rewritten"] += 1
            # through the ingest and bookkeeping of a poll's packets; when they arrived is what the heartbeat goes by, not when
            # they are mapped
            self._ingest_packets(0, m, now, held=(buf, np.array([p[2] for p in flat], dtype=np.uint16),
                                                  np.array([p[3] for p in flat], dtype=np.float64), [p[4] for p in flat]))

    def flush_trails(self, now=None):
        """match_packets: match and map everything pending, whatever its count or age."""
        if self.match_packets:
            now = time.time() if now is None else now
            self._flush_trails(now, True)
            for b in sorted(self._locating):         # still being located: what they hold is mapped as it is
                flat = self._locating.pop(b)[1]
                self.trail_stats["reloc_gave_up"] += 1
                if flat:
                    buf = np.zeros((len(flat), self.slot), dtype=np.uint8)
                    buf[:, :SLOT] = np.stack([p[1] for p in flat])
                    self._ingest_packets(0, len(flat), now, held=(buf, np.array([p[2] for p in flat], dtype=np.uint16),
                                                                  np.array([p[3] for p in flat], dtype=np.float64), [p[4] for p in flat]))

    def _note_checks(self, i0, checks, now):
        """check_sweeps: the checks of one guarded ingest whose first datagram is slot i0, in arrival order.  A withheld sweep
        still shows that its bot is there (address, heartbeat) but leaves its pose alone; a bot whose run of contradicted sweeps
        reaches lost_after loses its transform and is relocalised from its next sweep on, as a bot found offline is."""
        status = np.asarray(checks["status"])
        self._mark(i0, status == P.CHECK_CONTRADICTS, None, now, False)
        for j in np.nonzero(status != P.CHECK_NO_RECORD)[0]:
            a = int(self._buf[i0 + int(j), 4])
            self.check_stats["checked"] += 1
            if status[j] == P.CHECK_UNDECIDED:
                self.check_stats["undecided"] += 1
            elif status[j] == P.CHECK_OK:
                self.suspect[a] = 0
            else:
                self.check_stats["withheld"] += 1
                self.suspect[a] += 1
                if self.relocalise and self.suspect[a] >= self.lost_after and a not in self._lost:
                    self._lost.add(a)
                    self._reloc_T.pop(a, None)
                    self._reloc_kept.pop(a, None)

    def _runs(self, n):
        """Maximal runs of one kind in arrival order: (first, end, 0 for packets | the sweep stride)."""
        lens = self._lens[:n]
        kind = np.where((lens == P.PACKET_SIZE_V0) | (lens == P.PACKET_SIZE_V0_ODO), lens, 0).astype(np.int64)
        cuts = np.flatnonzero(np.diff(kind)) + 1
        starts = np.concatenate(([0], cuts))
        ends = np.concatenate((cuts, [n]))
        return [(int(a), int(b), int(kind[a])) for a, b in zip(starts, ends)]

    def _relocalise_run(self, run, lens):
        """relocalise: one run of sweeps (a view of the receive buffer) before its ingest.  The bots whose first acceptable
        record of the run finds them offline are relocalised on that record; then the records of every bot with a transform
        in force get their pose fields rewritten in place."""
        ok = ((lens == run.shape[1]) & (run[:, :4] == np.frombuffer(b"QSRL", dtype=np.uint8)).all(axis=1)
              & (run[:, 4] >= 1) & (run[:, 4] <= self.max_agent))
        idx = np.nonzero(ok)[0]
        first = {}
        for j in idx:
            a = int(run[j, 4])
            if (not self.online[a] or a in self._lost) and a not in first:
                first[a] = int(j)
        shift_of = getattr(self.mapper, "sweep_pose_shift", None)
        located = []                                 # (bot, the record whose ingest pose the transform starts from, the result)
        if self.reloc_group:
            located = self._relocalise_groups(run, idx, first)
        else:
            for a, j in first.items():
                r = self.mapper.relocalise_sweeps(run[j:j + 1], lens[j:j + 1], params=self.reloc_params)[0]
                self.reloc_stats["tried"] += 1
                if r["accepted"]:
                    located.append((a, run[j], r))
        for a, rec, r in located:
            x, y, yaw = (float(v) for v in rec[5:17].view("<f4"))
            sx, sy = (float(v) for v in shift_of(a)) if shift_of else (0.0, 0.0)
            dyaw = float(r["yaw"]) - yaw
            self._reloc_T[a] = (np.cos(dyaw), np.sin(dyaw), dyaw, x + sx, y + sy, float(r["x"]), float(r["y"]), sx, sy)
            self.relocalised[a] = r.copy()
            self.reloc_stats["accepted"] += 1
            if a in self._lost:                      # (check_sweeps) located again: its run starts anew
                self._lost.discard(a)
                self.suspect[a] = 0
        for j in idx:
            T = self._reloc_T.get(int(run[j, 4]))
            if T is None:
                continue
            c, s, dyaw, ix, iy, fx, fy, sx, sy = T
            f = run[j, 5:17].view("<f4")
            qx, qy = float(f[0]) + sx - ix, float(f[1]) + sy - iy
            f[:] = (fx + (c * qx - s * qy) - sx, fy + (s * qx + c * qy) - sy, float(f[2]) + dyaw)
            self.reloc_stats["rewritten"] += 1

    def _relocalise_groups(self, run, idx, first):
        """Group mode: keep this run's sweeps of the bots that are being located and relocalise each bot that got one more.
        first: the bots this run finds offline (they start anew unless they have a transform or are already being located)."""
        for a in first:
            if a not in self._reloc_T and a not in self._reloc_kept:
                self._reloc_kept[a] = []
        grew = set()
        for j in idx:
            a = int(run[j, 4])
            kept = self._reloc_kept.get(a)
            if kept is None or len(kept) >= self.reloc_group:
                continue
            if kept:
                if len(kept[0]) != run.shape[1]:
                    continue                          # (the other sweep format: one stride per call)
                x0, y0 = (float(v) for v in kept[0][5:13].view("<f4"))
                x, y = (float(v) for v in run[j, 5:13].view("<f4"))
                if not (x - x0) * (x - x0) + (y - y0) * (y - y0) <= self.reloc_travel * self.reloc_travel:
                    continue
            kept.append(run[j].copy())
            grew.add(a)
        located = []
        for a in sorted(grew):
            kept = self._reloc_kept[a]
            recs = np.stack(kept)
            r = self.mapper.relocalise_groups(recs, [len(kept)], np.full(len(kept), recs.shape[1], dtype=np.uint16),
                                              travel=self.reloc_travel, params=self.reloc_params)[0]
            self.reloc_stats["group_tried"] += 1
            if r["accepted"]:
                located.append((a, kept[0], r))
                del self._reloc_kept[a]
            elif len(kept) >= self.reloc_group:
                self.reloc_stats["gave_up"] += 1
                del self._reloc_kept[a]
        return located

    def _mark(self, i0, accepted, pose, now, keep_pose, buf=None, addrs=None, heartbeat=True):
        """Bookkeeping of the accepted records of one ingest whose first datagram is slot i0 (:846-848, :860-864) of the receive
        buffer, or of buf / addrs.  heartbeat=False (held packets, mapped later than they arrived): the count and the pose only."""
        buf = self._buf if buf is None else buf
        addrs = self._addrs if addrs is None else addrs
        for j in np.nonzero(accepted)[0]:
            i = i0 + int(j)
            a = int(buf[i, 4])
            self.pkt_counts[a] += 1                                                   # :848
            if heartbeat:
                self.bot_addrs[a] = (addrs[i][0], self.bot_ports[a])                  # :846
                self.last_packet_time[a] = now                                        # :847
                self.online[a] = True                                                 # :860-864
                self.seen[a] = True
            if keep_pose:
                self.bot_pose[a] = (float(pose[j, 0]), float(pose[j, 1]))

    def _track(self, i0, accepted, pose, buf=None):
        """track_view: the renderer's inputs of the accepted packets of one ingest (:878-879 the path, :892 the clouds)."""
        buf = self._buf if buf is None else buf
        xy, valid = self.mapper.last_hits()
        for j in np.nonzero(accepted)[0]:
            a = int(buf[i0 + int(j), 4])
            self.paths[a][0].append(float(pose[j, 0]))
            self.paths[a][1].append(float(pose[j, 1]))
            for s, name in enumerate(P.SENSOR_NAMES):
                if valid[j, s]:
                    self.point_clouds[a][name].append((float(xy[j, s, 0]), float(xy[j, s, 1])))

    # ---- :805-812 --------------------------------------------------------------------------------
    def heartbeat(self, now=None):
        now = time.time() if now is None else now
        went_offline = []
        for b in self.online:
            if self.seen[b] and self.last_packet_time[b] > 0 and now - self.last_packet_time[b] > P.HEARTBEAT_TIMEOUT:
                if self.online[b]:
                    self.online[b] = False
                    went_offline.append(b)
                    if self.bot_veil:
                        self.mapper.bot_veil_forget(b)
        return went_offline

    def other_of(self, bot_id):
        """The reference pairs bot 1 with bot 2 (:926); larger swarms are paired (1,2), (3,4), ..."""
        return bot_id + 1 if bot_id % 2 == 1 else bot_id - 1

    # ---- :922-945 --------------------------------------------------------------------------------
    def zone_tick(self, now=None, force=False):
        """Send every bot its partner's zone if the 2 s interval has elapsed.  Returns {bot: datagram}."""
        now = time.time() if now is None else now
        if not force and not (now - self.last_zone_send > P.ZONE_UPDATE_INTERVAL):    # :922
            return {}
        self.last_zone_send = now
        sent = {}
        for bot_id in self.online:
            other = self.other_of(bot_id)
            if other not in self.online:
                continue
            online = self.online.get(other, False)                                     # :929
            pkt = self.mapper.zone_packet(other, online=online)                       # :940-941 / :944-945
            self.zone_boxes[other] = self.mapper.zone(other) if online else None
            if self.bot_addrs[bot_id] is not None:                                    # send_zone_to_bot :677-678
                try:
                    self.sock.sendto(pkt, self.bot_addrs[bot_id])
                except OSError:
                    pass
            sent[bot_id] = pkt
        return sent

    # ---- :947-996 (the assignment and send the reference ships commented out) --------------------------------------
    def target_tick(self, now=None, force=False):
        """Every > TARGET_INTERVAL s: assign frontier targets to the online bots and send each assigned bot TARG
        (to its address if known).  Returns {bot: datagram} of the assigned bots."""
        now = time.time() if now is None else now
        if not force and not (now - self.last_target_send > P.TARGET_INTERVAL):
            return {}
        self.last_target_send = now
        states = {b: self.bot_pose[b] for b in sorted(self.online) if self.online[b] and self.bot_pose[b] is not None}
        if not states:
            return {}
        sent = {}
        if self.targets_by_path or self.targets_by_gain or self.targets_by_territory:
            targets = self._targets_by_cost(states)
        else:
            targets = sorted(self.mapper.assign_frontier_targets(states).items())
            if self.plan_paths and targets:
                targets = self._waypoints(states, targets)
        for bot_id, (tx, ty) in targets:
            pkt = P.pack_target(tx, ty)
            if self.bot_addrs[bot_id] is not None:                                    # send_target_to_bot :693-694
                try:
                    self.sock.sendto(pkt, self.bot_addrs[bot_id])
                except OSError:
                    pass
            sent[bot_id] = pkt
        return sent

    def _waypoints(self, states, targets):
        """One plan_paths call from the bots' poses to their centroids: the waypoint where the status is OK, else the
        centroid (what the reference would send); both counted in plan_stats."""
        res = self.mapper.plan_paths([states[b] for b, _ in targets], [xy for _, xy in targets], **self.plan_params)
        out = []
        for i, (b, xy) in enumerate(targets):
            if int(res["status"][i]) == 0:
                out.append((b, (float(res["waypoint"][i, 0]), float(res["waypoint"][i, 1]))))
                self.plan_stats["waypoint"] += 1
            else:
                out.append((b, xy))
                self.plan_stats["centroid"] += 1
        return out

    def _targets_by_cost(self, states):
        """One call that ranks the centroids by path cost (targets_by_gain: by gain over path cost; targets_by_territory: within
        each bot's share of the partitioned free space): the centroids of the assigned bots, or (plan_paths) their
        waypoints, which always exist; counted in plan_stats as _waypoints counts them.  targets_by_territory keeps
        territory = {bot: (cells owned, world box or None)}."""
        if self.targets_by_territory:
            kw = dict(by_territory=True, return_territory=True, **self.plan_params)
        elif self.targets_by_gain:
            kw = dict(by_gain=True, **self.plan_params, **self.gain_params)
        else:
            kw = dict(by_path=True, **self.plan_params)
        res = self.mapper.assign_frontier_targets(states, return_waypoints=self.plan_paths, **kw)
        res = res if isinstance(res, tuple) else (res,)
        if self.targets_by_territory:
            m = self.mapper
            self.territory = {
                b: (area, None if box is None else (m.ox + box[0] * m.res, m.oy + box[1] * m.res,
                                                    m.ox + (box[2] + 1) * m.res, m.oy + (box[3] + 1) * m.res))
                for b, (area, box) in res[-1].items()}
        if not self.plan_paths:
            return sorted(res[0].items())
        self.plan_stats["waypoint"] += len(res[1])
        return sorted(res[1].items())

    def step(self, now=None):
        """One iteration of the reference's while-loop body (without events and rendering)."""
        now = time.time() if now is None else now
        self.heartbeat(now)
        n = self.poll(now)
        self.zone_tick(now)
        if self.frontier_targets:
            self.target_tick(now)
        return n

    def run(self, duration, idle_sleep=0.001):
        end = time.time() + duration
        while time.time() < end:
            if self.step() == 0:
                time.sleep(idle_sleep)

    def close(self):
        """match_packets: what is pending is matched and mapped first, so close the front-end BEFORE its mapper; held packets of
        a mapper that is already closed (QuasarMapper: no handle left) are dropped."""
        if getattr(self.mapper, "_h", True):
            self.flush_trails()
        self.sock.close()
