"""The receive chain's plan restated in Python integers (include/sdrainer_hip.h "receive chain", csrc/host/chain_plan.h): the
oracle of tests/test_chain_plan.py and tests/test_chain_gpu.py.  What a push uploads, which pieces it processes and where
their outputs land in the ring, when the carry moves and which bank batches follow are a function of the geometry and the
push lengths alone; this module computes them, prints them in the format of tests/host/test_chain_plan.cpp, draws that
program's seeded geometries and push lengths with the same generator, and checks the invariants a trace must keep.  A plain
helper module, not a test file."""
from math import gcd


def lcm(a, b):
    return a // gcd(a, b) * b


def granule(total_decimation, nb_block=1):
    """G = lcm(2 * Dtot, nb block, 16); -1 for an argument below 1."""
    if total_decimation < 1 or nb_block < 1:
        return -1
    return lcm(lcm(2 * total_decimation, nb_block), 16)


def piece(g, limit):
    """The largest multiple of G within the smallest member capacity (in wide samples); 0: none fits."""
    if g < 1 or limit < 1:
        return -1
    return limit // g * g


def min_ring(block_size, hop, piece_, total_decimation):
    """2 * block_size + piece / Dtot rounded up to 4; -1 for an illegal argument."""
    if block_size < 1 or hop < 1 or hop > block_size or piece_ < 1 or total_decimation < 1 or piece_ % total_decimation:
        return -1
    return (2 * block_size + piece_ // total_decimation + 3) // 4 * 4


class Plan:
    """The chain's state machine.  limit: the smallest of the members' max_in_samples in wide samples (the fine converter's
    times stage one's decimation); ring = 0 takes the minimum.  push() returns the actions as tuples:
        ("upload", raw offset, samples)            host pushes only: behind the pending samples
        ("move", source, destination, samples)     the ring's unconsumed samples to its front (samples may be 0)
        ("piece", input offset, wide samples, ring offset of its outputs)
        ("batch", ring offset of the first frame, frames)
        ("keep", source, destination, samples)     what stays pending, to the raw buffer's front"""

    def __init__(self, total_decimation, nb_block, limit, block_size, hop, max_batch_frames, max_in, ring=0):
        self.dtot, self.block, self.hop, self.max_batch, self.max_in = total_decimation, block_size, hop, max_batch_frames, max_in
        self.g = granule(total_decimation, nb_block)
        self.piece = piece(self.g, limit)
        assert self.piece >= self.g > 0
        self.min_ring = min_ring(block_size, hop, self.piece, total_decimation)
        self.ring = ring or self.min_ring
        assert self.ring >= self.min_ring and self.ring % 4 == 0
        self.accepted = self.processed = self.pending = 0  # wide samples
        self.base = self.have = 0                            # the ring holds narrow samples [base, have)
        self.frames = self.batches = self.moves = 0

    def check(self, n, host):
        """None, or why the push is refused: "size" (SDR_ERR_BAD_SIZE) or "state" (SDR_ERR_STATE)."""
        if n < 1 or n > self.max_in or (not host and n % self.g):
            return "size"
        if not host and self.pending:
            return "state"
        return None

    def push(self, n, host):
        assert self.check(n, host) is None
        out = []
        avail = self.pending + n
        if host:
            out.append(("upload", self.pending, n))
        self.accepted += n
        whole = avail // self.g * self.g
        off = 0
        while off < whole:
            p = min(self.piece, whole - off)
            m = p // self.dtot
            if self.have - self.base + m > self.ring:
                nxt = self.frames * self.hop
                out.append(("move", nxt - self.base, 0, self.have - nxt))
                self.base = nxt
                self.moves += 1
            out.append(("piece", off, p, self.have - self.base))
            self.have += m
            off += p
            self.processed += p
            while self.have - self.frames * self.hop >= self.block:
                nxt = self.frames * self.hop
                f = min((self.have - nxt - self.block) // self.hop + 1, self.max_batch)
                out.append(("batch", nxt - self.base, f))
                self.frames += f
                self.batches += 1
        self.pending = avail - whole
        if host and whole > 0 and self.pending > 0:
            out.append(("keep", whole, 0, self.pending))
        return out

    def state(self):
        return (self.accepted, self.processed, self.pending, self.base, self.have, self.frames, self.batches, self.moves)


def batches_of(plan, n, host=True):
    """Pushes n samples and returns the bank batches the push enqueues as (first frame, frames) pairs."""
    first = plan.frames
    out = []
    for a in plan.push(n, host):
        if a[0] == "batch":
            out.append((first, a[2]))
            first += a[2]
    return out


# -- the seeded cases of tests/host/test_chain_plan.cpp, drawn with the same generator --------------------------------------
class SplitMix:
    """splitmix64, as in the C++ program."""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def below(self, n):
        return self.next() % n


DTOTS = (1, 2, 3, 5, 8, 12, 32, 100, 256, 1000, 4096, 8192)
NB_BLOCKS = (1, 64, 96, 256, 4096)
MAX_BATCH = (3, 7, 64, 1024)
SEED, GEOMETRIES, PUSHES = 20_250_117, 160, 48


def draw_geometry(rng):
    """dict of the Plan's arguments: block 512 .. 8192, hop block / 16 .. block, Dtot 1 .. 8192 (the listed ones or any), nb
    blocks including 96, a member capacity that is no multiple of G, a push capacity from below G to above three pieces."""
    block = 512 << rng.below(5)
    hop = block >> rng.below(5)
    dtot = DTOTS[rng.below(len(DTOTS))] if rng.below(2) else 1 + rng.below(8192)
    nb = NB_BLOCKS[rng.below(len(NB_BLOCKS))]
    g = granule(dtot, nb)
    limit = g * (1 + rng.below(6)) + rng.below(g)
    pc = piece(g, limit)
    max_in = 1 + rng.below(3 * pc + 17)
    max_batch = MAX_BATCH[rng.below(len(MAX_BATCH))]
    ring = min_ring(block, hop, pc, dtot)
    if rng.below(2):
        ring += 4 * rng.below(ring // 2)
    return dict(total_decimation=dtot, nb_block=nb, limit=limit, block_size=block, hop=hop, max_batch_frames=max_batch, max_in=max_in, ring=ring)


def draw_push(rng, plan):
    """(n, host): lengths of 1, below G, the capacity and anything between; one push in four is a device push of whole
    granules (refused while samples are pending, or where not one granule fits the capacity)."""
    kind = rng.below(8)
    if kind < 2:
        return plan.g * (1 + rng.below(max(1, plan.max_in // plan.g))), False
    if kind == 2:
        return 1, True
    if kind == 3:
        return 1 + rng.below(plan.g), True
    if kind == 4:
        return plan.max_in, True
    return 1 + rng.below(plan.max_in), True


def trace(seed=SEED, geometries=GEOMETRIES, pushes=PUSHES):
    """The lines tests/host/test_chain_plan.cpp prints, and per geometry the Plan's arguments with the actions of every push
    (for check_invariants)."""
    rng = SplitMix(seed)
    lines, cases = [], []
    for i in range(geometries):
        geo = draw_geometry(rng)
        plan = Plan(**geo)
        lines.append("geom %d dtot %d nb %d granule %d piece %d ring %d block %d hop %d max_batch %d max_in %d" % (
            i, plan.dtot, geo["nb_block"], plan.g, plan.piece, plan.ring, plan.block, plan.hop, plan.max_batch, plan.max_in))
        log = []
        for _ in range(pushes):
            n, host = draw_push(rng, plan)
            lines.append("push %d %s" % (n, "host" if host else "device"))
            why = plan.check(n if n <= plan.max_in else plan.max_in + 1, host)
            if why:
                lines.append("refuse " + why)
                continue
            actions = plan.push(n, host)
            for a in actions:
                lines.append(" ".join(str(v) for v in a))
            lines.append("state " + " ".join(str(v) for v in plan.state()))
            log.append((n, host, actions, plan.state()))
        cases.append((geo, log))
    return lines, cases


def parse(lines):
    """A printed trace back into [(geometry dict, [(n, host, actions, state)])]: what check_invariants takes."""
    cases = []
    for ln in lines:
        w = ln.split()
        if w[0] == "geom":
            v = dict(zip(w[2::2], (int(x) for x in w[3::2])))
            cases.append((v, []))
        elif w[0] == "push":
            cur = [int(w[1]), w[2] == "host", [], None]
        elif w[0] == "refuse":
            cur = None
        elif w[0] == "state":
            cur[3] = tuple(int(x) for x in w[1:])
            cases[-1][1].append(tuple(cur))
        else:
            cur[2].append((w[0],) + tuple(int(x) for x in w[1:]))
    return cases


def check_invariants(cases):
    """Over parsed traces (geometry keys as printed): every stage pointer offset is even and every piece starts on a granule;
    a carry move and a pending move never overlap; nothing is written past the ring or the raw buffer; a batch reads only
    samples that were written; fewer than block_size samples are unconsumed after a piece's batches; processed + pending ==
    accepted.  Returns (pieces, carry moves, batches, pending moves) seen, so that a caller can insist they occurred."""
    seen = dict(piece=0, move=0, batch=0, keep=0, empty_move=0)
    for geo, log in cases:
        g, dtot, ring, block, hop = geo["granule"], geo["dtot"], geo["ring"], geo["block"], geo["hop"]
        assert g % (2 * dtot) == 0 and g % geo["nb"] == 0 and g % 16 == 0 and geo["piece"] % g == 0 and geo["piece"] >= g
        base = have = frames = pending = accepted = processed = 0
        for n, host, actions, state in log:
            filled = pending + (n if host else 0)  # samples the raw buffer holds for this push
            accepted += n
            for i, a in enumerate(actions):
                seen[a[0]] = seen.get(a[0], 0) + 1
                if a[0] == "upload":
                    assert host and i == 0 and a[1] == pending and a[2] == n and a[1] + a[2] <= g - 1 + geo["max_in"], (geo, a)
                elif a[0] == "move":
                    _, src, dst, ln = a
                    assert dst == 0 and src == frames * hop - base and ln == have - frames * hop, (geo, a)
                    assert 0 <= ln < block and src >= dst + ln and src % 2 == 0, ("the carry move overlaps", geo, a)
                    seen["empty_move"] += ln == 0
                    base = frames * hop
                elif a[0] == "piece":
                    _, off, p, at = a
                    m = p // dtot
                    assert p % g == 0 and 0 < p <= geo["piece"] and off % g == 0 and m % 2 == 0, (geo, a)
                    assert off + p <= (filled if host else n), ("a piece reads past the samples that are there", geo, a)
                    assert at == have - base and at % 2 == 0 and at + m <= ring, ("a piece writes past the ring", geo, a)
                    assert have - frames * hop < block, ("a piece starts with a whole frame unconsumed", geo, a)
                    have += m
                    processed += p
                    nxt = actions[i + 1] if i + 1 < len(actions) else None
                    if nxt is None or nxt[0] != "batch":
                        assert have - frames * hop < block, ("a frame is left behind a piece", geo, a)
                elif a[0] == "batch":
                    _, at, f = a
                    assert at == frames * hop - base and at % 2 == 0 and 1 <= f <= geo["max_batch"], (geo, a)
                    assert at + (f - 1) * hop + block <= have - base <= ring, ("a batch reads past the samples written", geo, a)
                    frames += f
                    nxt = actions[i + 1] if i + 1 < len(actions) else None
                    if nxt is None or nxt[0] != "batch":
                        assert have - frames * hop < block, ("a frame is left behind a piece's batches", geo, a)
                    else:
                        assert f == geo["max_batch"], ("a short batch with frames left", geo, a)
                elif a[0] == "keep":
                    _, src, dst, ln = a
                    assert host and i == len(actions) - 1 and dst == 0 and 0 < ln < g and src >= dst + ln and src % g == 0, (geo, a)
                    assert src + ln == filled, (geo, a)
                else:
                    raise AssertionError(a)
            pending = accepted - processed
            assert 0 <= pending < g and (host or pending == 0), (geo, n, host)
            want = (accepted, processed, pending, base, have, frames)
            assert state[:6] == want, (geo, state, want)
    return seen
