"""The draw the two RANSAC units share, restated in Python for tests/two_view_ref.py and tests/sim3_ref.py, independently of csrc/ransac_draw.h: the library's stand-in for
rand() (include/sslam_frontend.h) and the reference's swap-with-back (src/Initializer.cc:93-108, src/Sim3Solver.cc:163-177) given the random integers."""
M32 = 0xFFFFFFFF


def mix32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32; x ^= x >> 15; x = (x * 0x846ca68b) & M32; x ^= x >> 16
    return x


def hash32(seed, pair, it, j):
    return mix32(mix32(mix32(mix32(seed + 0x9e3779b9) ^ pair) ^ it) ^ j)


def draw(n, randi):
    """one iteration: vAvailableIndices = all n indices; for every randi[j] = RandomInt(0, vAvailableIndices.size() - 1) take [randi[j]] and move the back into its place"""
    avail = list(range(n))
    out = []
    for r in randi:
        r = int(r)
        assert 0 <= r <= len(avail) - 1
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out
