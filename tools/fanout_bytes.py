"""Upload bytes per batch of readpath_test --bench's level multi-gets, from sizes
(replays Queries() and the level geometry: 16 tables, stride 50000, span 200000)."""
M = (1 << 64) - 1
T, stride, span = 16, 50000, 200000
key_space = stride * (T - 1) + span
for batch in (1000, 65536):
    s = 11 + batch
    K = P = key_bytes = pair_key_bytes = 0
    for i in range(batch):
        s = (s * 6364136223846793005 + 1442695040888963407) & M
        r = s >> 17
        if i % 3 == 2:
            n, ln, hash_ = r % key_space, 14, True
        elif i % 11 == 10:
            n, ln, hash_ = None, 3 + len(str(r)), False
        else:
            n, ln, hash_ = r % key_space, 13, False
        fan = 0
        if n is not None:
            for t in range(T):
                lo, hi = t * stride, t * stride + span
                # "userN#" sorts after userN and before user(N+1): covered when lo <= N < hi - 1
                if lo <= n and (n < hi - 1 if hash_ else n <= hi - 1):
                    fan += 1
        K += 1
        P += fan
        key_bytes += ln
        pair_key_bytes += fan * ln
    pair_up = pair_key_bytes + 8 * (P + 1) + 4 * P
    fan_up = key_bytes + 8 * (K + 1) + 4 * (K + 1) + 4 * P
    print(batch, "pairs", P, "pair path upload", pair_up, "fan-out upload", fan_up, "saved", pair_up - fan_up,
          "answers back", P)
