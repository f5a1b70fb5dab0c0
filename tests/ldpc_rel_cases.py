"""The LDPC decoder's byte reliabilities as NumPy and plain Python, shared by test_ldpc_rel_host.py, test_gpu_ldpc_rel.py
and tools/ldpc_rel_gain.py.  ``code(rate)`` is ldpc_rate_cases' model of the rate whose decoder also returns, per
codeword, the values P it held when the codeword stopped and whether its checks were open; ``rel`` turns them into one
reliability byte per payload byte, one Python integer at a time.  Restates include/ofdm_hip.h ("coded links: LDPC,
reliabilities out"):

    q[g] = min(127, min over the eight bits of |P[8m + i]|) + 128 * conv

for payload byte g of the block, info byte m of its codeword.  Everything is integer arithmetic, so a GPU result is
compared by equality."""
import functools

import numpy as np

import ldpc_rate_cases as lr
import rs_cases as rc
import rs_rel_cases as rr

RATES = lr.RATES
DEFAULT_ITERS = lr.DEFAULT_ITERS
NO_BLOCK = lr.NO_BLOCK + (np.zeros(0, np.uint8),)
CHAIN_PAYLOAD = 880              # the seeded chain below: four RS codewords in eleven rate-1/2 LDPC codewords
CHAIN_M = 28
# (rate, Eb/N0 dB) -> the seeds of 0 .. 119 that only the reliabilities return, RS alone / with them returned
CHAIN_POINTS = {("1/2", 1.5): ((20, 28, 44, 54, 67), 108, 113), ("3/4", 2.5): ((5, 11, 77), 71, 74)}


class Code(lr.Code):
    """ldpc_rate_cases.Code with the decoder's final state kept."""

    def decode_codewords_rel(self, v, max_iters=DEFAULT_ITERS):
        """decode_codewords that also returns P: v [W, 1536] -> (bits, iters, failed, P int32 [W, 1536]), P and failed
        frozen at the iteration the codeword stopped, as bits are."""
        v = np.asarray(v, np.int32)
        W = v.shape[0]
        P = v.copy()
        R = [np.zeros((W, len(row), lr.Z), np.int32) for row in self.ROW_ENTRIES]
        bits = np.zeros((W, lr.N_BITS), np.uint8)
        iters = np.zeros(W, np.int64)
        failed = np.ones(W, bool)
        act = np.arange(W)
        for it in range(1, max_iters + 1):
            if len(act) == 0:
                break
            Pa = P[act]
            for i, idx in enumerate(self.ROW_INDEX):
                d = len(idx)
                Q = np.clip(Pa[:, idx] - R[i][act], -127, 127)
                beta = Q > 0
                par = np.bitwise_xor.reduce(beta, axis=1)
                mag = np.abs(Q)
                two = np.partition(mag, 1, axis=1)[:, :2]
                m1, m2 = two[:, 0], two[:, 1]
                pos = np.argmin(mag, axis=1)
                others = np.where(np.arange(d)[None, :, None] == pos[:, None, :], m2[:, None, :], m1[:, None, :])
                Rn = np.where(par[:, None, :] ^ beta, (3 * others) >> 2, -((3 * others) >> 2))
                R[i][act] = Rn
                Pa[:, idx] = Q + Rn
            P[act] = Pa                      # a codeword that stops here leaves ``act``: its P stays as it is now
            x = (Pa > 0).astype(np.uint8)
            bad = self.syndrome(x).reshape(len(act), -1).any(axis=1)
            bits[act] = x
            iters[act] = it
            failed[act] = bad
            act = act[bad]
        return bits, iters, failed, P

    def rel(self, P, failed, k):
        """The n = k - 4 reliability bytes of a block with k info bytes from its codewords' P [W, 1536] and failed [W],
        straight from the definition."""
        KI = self.CW_INFO
        q = []
        for g in range(k - 4):
            w, m = divmod(g, KI)
            weakest = min(abs(int(P[w][8 * m + i])) for i in range(8))
            q.append(min(127, weakest) + (0 if failed[w] else 128))
        return np.array(q, np.uint8).reshape(-1)

    def decode_many_rel(self, values, max_iters=DEFAULT_ITERS):
        """decode_many with reliabilities: (ok, payload, corrected, iters, cw_failed, rel uint8 [len(payload)]) per block."""
        out = [None] * len(values)
        parts = []
        for i, v in enumerate(values):
            v = np.asarray(v, np.int8)
            if len(v) % 8 or not self.is_block(len(v) // 8):
                out[i] = NO_BLOCK
            else:
                parts.append((i,) + self.block_values(v))
        if not parts:
            return out
        bits, iters, failed, P = self.decode_codewords_rel(np.concatenate([p[1] for p in parts]), max_iters)
        o = 0
        for i, V, sent, k in parts:
            s = slice(o, o + len(V))
            out[i] = self._result(V, sent, k, bits[s], iters[s], failed[s]) + (self.rel(P[s], failed[s], k),)
            o += len(V)
        return out

    def decode_values_rel(self, v, max_iters=DEFAULT_ITERS):
        return self.decode_many_rel([v], max_iters)[0]

    def decode_rel(self, block, max_iters=DEFAULT_ITERS):
        """One hard block (bytes of any length) -> the six fields."""
        block = bytes(block)
        if not self.is_block(len(block)):
            return NO_BLOCK
        return self.decode_values_rel(lr.hard_values(block), max_iters)


@functools.lru_cache(maxsize=None)
def code(rate):
    return Code(rate)


def same(a, b):
    """Two six-field results (or lists of them) are equal, the reliabilities compared as arrays."""
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return tuple(a[:5]) == tuple(b[:5]) and np.asarray(a[5]).dtype == np.uint8 and np.array_equal(a[5], b[5])


def spoil(block, words, count=16, seed=1):
    """The hard block with ``count`` sent bits flipped in each of the full codewords ``words``: with 16 the codeword's
    checks are still open after one iteration and closed after two or three, at every rate (the tests assert it)."""
    pos = np.random.default_rng(seed).choice(8 * lr.CW_SENT, count, replace=False)
    return lr.flip(block, np.concatenate([8 * lr.CW_SENT * w + pos for w in words]))


# ---- the seeded chain: RS above LDPC over BPSK / AWGN, one default_rng(seed) per block --------------------------------
def chain_block(seed, rate="1/2", ebn0_db=1.5, n=CHAIN_PAYLOAD):
    """(payload, values) of one seeded block: payload -> RS -> LDPC at ``rate`` -> int8 values at Eb/N0."""
    c = code(rate)
    rng = np.random.default_rng(seed)
    payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    block = c.encode(rc.encode(payload))
    return payload, c.awgn_values(block, ebn0_db, rng)


def chain_outer(decoded, q, M=CHAIN_M):
    """The RS model on an inner decoder's bytes without and with its reliabilities: (rs_cases.decode's four fields,
    rs_rel_cases.decode's five)."""
    return rc.decode(decoded), rr.decode(decoded, q, M)


@functools.lru_cache(maxsize=None)
def chain(seeds, rate="1/2", ebn0_db=1.5):
    """Per seed (payload, values, the model's six fields, RS alone, RS with the reliabilities), computed once."""
    c = code(rate)
    blocks = [chain_block(s, rate, ebn0_db) for s in seeds]
    inner = c.decode_many_rel([v for _, v in blocks])
    return tuple((p, v, d) + chain_outer(d[1], d[5]) for (p, v), d in zip(blocks, inner))
