"""Shared by the planner tests: an independent numpy restatement of the categorical cross-entropy method of csrc/plan.hip
(include/srlz.h states it) — Philox4x32-10, the sampler, select, refit, the best-so-far rule and the whole loop over a
`returns_fn(plans)`.  Everything but the returns is integer arithmetic, so every comparison against it is exact.
It imports nothing of srlz.deploy's implementation, touches no GPU and reads no file."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SHIFT = np.uint64(32)
# counter, key, output of Philox4x32-10 (the known answers of the Random123 distribution)
PHILOX_KATS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
               ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox(counter, key):
    """Philox4x32-10.  counter: four integers or integer arrays (broadcast together), key: two integers.  Returns four uint64 arrays
    holding 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 bits: exact in 64
        c = [(p1 >> SHIFT) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> SHIFT) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def pick(u, cum_row):
    """The action of one 32-bit draw u on one table row: the first a with cum[a] > (u * cum[A-1]) >> 32."""
    row = [int(v) for v in cum_row]
    target = (int(u) * row[-1]) >> 32
    for a, v in enumerate(row):
        if v > target:
            return a
    raise AssertionError("a row without a positive total")


def uniform_cum(n, t, a):
    return np.tile(np.arange(1, a + 1, dtype=np.uint32), (n, t, 1))


def cum_of(weights, n):
    """uint32 [n,T,A] table of integer weights [T,A] or [n,T,A]."""
    w = np.asarray(weights).astype(np.uint64)
    if w.ndim == 2:
        w = np.broadcast_to(w, (n,) + w.shape)
    return np.cumsum(w, axis=2).astype(np.uint32)


def sample(cum, seed, iteration, k, n0=0, k0=0):
    """int32 [N,K,T]: the plans of one iteration from the table cum [N,T,A]; n0 / k0 offset the environment / plan numbers."""
    cum = np.asarray(cum).astype(np.uint64)
    n, t, a = cum.shape
    ni, ki, ti = np.meshgrid(np.arange(n) + n0, np.arange(k) + k0, np.arange(t), indexing="ij")
    words = philox((ti >> 2, ki, ni, np.full_like(ti, iteration)), (seed & 0xFFFFFFFF, seed >> 32))
    u = np.choose(ti & 3, words)
    total = cum[:, :, a - 1][:, None, :]                      # [N,1,T]
    target = (u * total) >> SHIFT                              # below 2^64: both factors are below 2^32
    return (cum[:, None, :, :] <= target[..., None]).sum(axis=3).astype(np.int32)  # rows do not decrease: the first entry above


def select(returns, elites):
    """Indices of the elites of one environment's returns [K]: key = the return, NaN as -inf; key descending, then k ascending."""
    key = np.asarray(returns, np.float32).copy()
    key[np.isnan(key)] = -np.inf
    order = sorted(range(len(key)), key=lambda k: (-float(key[k]), k))
    return np.array(order[:elites]), key


def refit(elite_plans, a, q):
    """uint32 [T,A]: prefix sums of 1 + q * count[t][a] over the elites' plans [E,T]."""
    e, t = elite_plans.shape
    w = np.ones((t, a), np.uint64)
    for row in elite_plans:
        for step, action in enumerate(row):
            w[step, action] += np.uint64(q)
    return np.cumsum(w, axis=1).astype(np.uint32)


def cem(returns_fn, n, k, t, a, iterations, elites, q, seed, init_weights=None, given=None):
    """The whole planner over returns_fn(plans int32 [N,K,T]) -> fp32 [N,K].  `given`: a list of per-iteration returns to use
    instead of calling returns_fn (a recorded run).  Returns a dict: plans [I,N,K,T], returns [I,N,K], cums [I+1,N,T,A] (the table
    each iteration sampled from, then the final one), best_plan [N,T], best_return [N], history [I,N] (best key so far)."""
    cum = uniform_cum(n, t, a) if init_weights is None else cum_of(init_weights, n)
    cums, pops, rets, hist = [cum.copy()], [], [], []
    best_plan, best_ret, best_key = np.zeros((n, t), np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i in range(iterations):
        pl = sample(cum, seed, i, k)
        r = np.asarray(given[i] if given is not None else returns_fn(pl), np.float32).reshape(n, k)
        cum = np.empty_like(cum)
        for e in range(n):
            el, key = select(r[e], elites)
            top = el[0]
            if i == 0 or key[top] > best_key[e]:
                best_key[e], best_ret[e], best_plan[e] = key[top], r[e, top], pl[e, top]
            cum[e] = refit(pl[e, el], a, q)
        pops.append(pl)
        rets.append(r)
        cums.append(cum.copy())
        hist.append(best_key.copy())
    return dict(plans=np.stack(pops), returns=np.stack(rets), cums=np.stack(cums), cum=cum, best_plan=best_plan, best_return=best_ret,
                history=np.stack(hist))


def weights_of(cum):
    """int64 weights of a table (the differences along the actions)."""
    return np.diff(np.asarray(cum).astype(np.int64), axis=-1, prepend=0)


def shifted(cum):
    """int64 weights for the controller's next call: step 0 dropped, a uniform last step."""
    w = weights_of(cum)
    return np.concatenate((w[..., 1:, :], np.ones_like(w[..., :1, :])), axis=-2)


TOY = dict(a=6, t=7, k=64, elites=8, q=8, iterations=6)


def toy_returns(plans):
    """The number of steps where the plan hits target[t] = (3 t + 1) mod 6."""
    t = plans.shape[-1]
    target = (3 * np.arange(t) + 1) % 6
    return (plans == target).sum(axis=-1).astype(np.float32)
