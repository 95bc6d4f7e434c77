"""CPU: ik_post_plan, the routing ik_transform_batch's post stage executes (csrc/ik_post_plan.h):
which launch resizes each request of a batch and which coder writes its file.  The
thresholds are the documented ones -- IK_WEBP_AUTO takes the exact GPU coder from 32
same-geometry frames on, one mixed exact call takes 32 WebP requests (2 under
IK_WEBP_EXACT) -- written out here, not read from the library.  Host only, no GPU."""
import ctypes
import random

from imagekit import _lib

JPEG, WEBP, AVIF = 0, 1, 2                      # ik_format
LIBWEBP, EXACT, AUTO = 0, 2, 3                  # ik_webp_encoder
MIX_HOST, MIX_GPU = 0, 1                        # ik_webp_mixed
NONE, SINGLE, MIXED, FRONT_GROUP, EXACT_GROUP, JPEG_GROUP = range(6)  # ik_post_route
GROUP_ROUTES = (FRONT_GROUP, EXACT_GROUP, JPEG_GROUP)
AUTO_MIN, MIXED_MIN = 32, 32


def req(W=64, H=48, C=3, pitch=256, device=0, depth=1, w=40, h=30, fmt=WEBP, q=80, ok=1):
    return dict(ok=ok, W=W, H=H, C=C, pitch=pitch, device=device, depth=depth, w=w, h=h, fmt=fmt, q=q)


class Plan:
    def __init__(self, reqs, enc, mix):
        m = len(reqs)
        n = max(m, 1)

        def arr(ct, key):
            return (ct * n)(*[r[key] for r in reqs])

        nw, nh = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
        rg, cg, route = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
        info = (ctypes.c_uint32 * 4)()
        rc = _lib.load().ik_post_plan(
            m, arr(ctypes.c_int, "ok"), arr(ctypes.c_uint32, "W"), arr(ctypes.c_uint32, "H"), arr(ctypes.c_uint32, "C"),
            arr(ctypes.c_uint64, "pitch"), arr(ctypes.c_int, "device"), arr(ctypes.c_uint32, "depth"),
            arr(ctypes.c_int64, "w"), arr(ctypes.c_int64, "h"), arr(ctypes.c_int, "fmt"), arr(ctypes.c_int, "q"),
            enc, mix, nw, nh, rg, cg, route, info)
        assert rc == 0
        self.reqs = reqs
        self.size = list(zip(nw, nh))[:m]
        self.rg, self.cg, self.route = list(rg)[:m], list(cg)[:m], list(route)[:m]
        self.mixed, self.mixed_min, self.n_rg, self.n_cg = bool(info[0]), info[1], info[2], info[3]
        self.check()

    def members(self, ids, g):
        return [k for k, v in enumerate(ids) if v == g]

    def rkey(self, k):
        r = self.reqs[k]
        return (r["W"], r["H"], r["C"], r["pitch"], r["device"]) + self.size[k]

    def check(self):
        """What holds for every plan."""
        reqs = self.reqs
        for k, r in enumerate(reqs):
            if not r["ok"]:
                assert (self.route[k], self.rg[k], self.cg[k]) == (NONE, -1, -1)
                continue
            assert self.route[k] in (SINGLE, MIXED) + GROUP_ROUTES  # exactly one route
            assert (self.route[k] in GROUP_ROUTES) == (self.cg[k] >= 0)
            assert -1 <= self.rg[k] < self.n_rg and -1 <= self.cg[k] < self.n_cg
            if self.cg[k] >= 0:
                assert self.rg[k] >= 0
            if self.route[k] == MIXED:
                assert self.mixed and r["fmt"] == WEBP and r["depth"] == 1
                assert all(1 <= d <= 16383 for d in self.size[k])
            if self.route[k] == EXACT_GROUP:
                assert all(d <= 16383 for d in self.size[k])
            if r["depth"] != 1:
                assert self.rg[k] == -1 and self.route[k] == SINGLE
        if not self.mixed:
            assert MIXED not in self.route
        keys = []
        for g in range(self.n_rg):
            ks = self.members(self.rg, g)
            assert len(ks) >= 2
            assert len({self.rkey(k) for k in ks}) == 1  # the members share the key
            assert self.size[ks[0]] != (reqs[ks[0]]["W"], reqs[ks[0]]["H"])  # all of them need a resize
            keys.append(self.rkey(ks[0]))
        assert keys == sorted(keys) and len(set(keys)) == len(keys)  # ascending key order
        ckeys = []
        for c in range(self.n_cg):
            ks = self.members(self.cg, c)
            assert len(ks) >= 2
            assert len({(reqs[k]["fmt"], reqs[k]["q"]) for k in ks}) == 1
            assert len({self.rg[k] for k in ks}) == 1  # inside one resize group
            assert len({self.route[k] for k in ks}) == 1
            fmt = reqs[ks[0]]["fmt"]
            assert (fmt == JPEG) == (self.route[ks[0]] == JPEG_GROUP) and fmt in (JPEG, WEBP)
            ckeys.append((self.rg[ks[0]], fmt != WEBP, reqs[ks[0]]["q"]))  # WebP before JPEG, by quality
        assert ckeys == sorted(ckeys) and len(set(ckeys)) == len(ckeys)

    def partition(self):
        """Groups as sets of request indices, and the per-request routes."""
        rgs = [tuple(self.members(self.rg, g)) for g in range(self.n_rg)]
        cgs = [tuple(self.members(self.cg, c)) for c in range(self.n_cg)]
        return rgs, cgs, self.route, self.size


def test_auto_threshold_mixed_host():
    p = Plan([req() for _ in range(AUTO_MIN)], AUTO, MIX_HOST)
    assert (p.n_rg, p.n_cg) == (1, 1) and p.route == [EXACT_GROUP] * 32 and not p.mixed
    assert p.size == [(40, 30)] * 32
    p = Plan([req() for _ in range(AUTO_MIN - 1)], AUTO, MIX_HOST)
    assert (p.n_rg, p.n_cg) == (1, 1) and p.route == [FRONT_GROUP] * 31


def test_auto_mixed_gpu():
    lone = req(W=100, H=80, pitch=512, w=50, h=40)
    p = Plan([req() for _ in range(31)] + [lone], AUTO, MIX_GPU)  # 32 candidates
    assert p.mixed and p.mixed_min == MIXED_MIN
    assert p.route == [MIXED] * 32 and p.n_rg == 1 and p.n_cg == 0
    assert p.rg == [0] * 31 + [-1]
    p = Plan([req() for _ in range(31)] + [lone], AUTO, MIX_HOST)
    assert not p.mixed and p.route == [FRONT_GROUP] * 31 + [SINGLE] and p.n_cg == 1
    p = Plan([req() for _ in range(30)] + [lone], AUTO, MIX_GPU)  # 31 candidates
    assert not p.mixed and p.route == [FRONT_GROUP] * 30 + [SINGLE]


def test_exact():
    third = req(W=100, H=80, pitch=512, w=50, h=40)
    p = Plan([req(), req(), third], EXACT, MIX_GPU)
    assert p.mixed and p.mixed_min == 2
    assert p.route == [EXACT_GROUP, EXACT_GROUP, MIXED] and p.cg == [0, 0, -1]
    p = Plan([req(), req(), third], EXACT, MIX_HOST)
    assert not p.mixed and p.mixed_min == 2
    assert p.route == [EXACT_GROUP, EXACT_GROUP, SINGLE]


def test_libwebp_never_exact_or_mixed():
    p = Plan([req() for _ in range(40)] + [req(w=-1, h=-1) for _ in range(40)], LIBWEBP, MIX_GPU)
    assert not p.mixed
    assert p.route == [FRONT_GROUP] * 40 + [SINGLE] * 40


def test_two_qualities_in_one_resize_group():
    rs = [req(), req(q=50), req(), req()]
    p = Plan(rs, EXACT, MIX_HOST)
    assert p.rg == [0, 0, 0, 0] and p.n_rg == 1 and p.n_cg == 1
    assert p.route == [EXACT_GROUP, SINGLE, EXACT_GROUP, EXACT_GROUP] and p.cg == [0, -1, 0, 0]
    p = Plan(rs, EXACT, MIX_GPU)
    assert p.rg == [0, 0, 0, 0] and p.route == [EXACT_GROUP, MIXED, EXACT_GROUP, EXACT_GROUP]


def test_jpeg_and_avif():
    p = Plan([req(fmt=JPEG, q=85), req(fmt=AVIF, q=60), req(fmt=JPEG, q=85), req(fmt=AVIF, q=60)], AUTO, MIX_HOST)
    assert p.rg == [0, 0, 0, 0] and p.n_cg == 1
    assert p.route == [JPEG_GROUP, SINGLE, JPEG_GROUP, SINGLE] and p.cg == [0, -1, 0, -1]
    # WebP groups come before JPEG ones, each by quality
    p = Plan([req(fmt=JPEG, q=85), req(q=90), req(fmt=JPEG, q=85), req(q=70), req(q=90), req(q=70)], LIBWEBP, MIX_HOST)
    assert p.cg == [2, 1, 2, 0, 1, 0]


def test_requests_needing_no_resize_join_no_group():
    for enc in (AUTO, EXACT):
        p = Plan([req(w=-1, h=-1) for _ in range(32)] + [req(w=64, h=48) for _ in range(32)], enc, MIX_HOST)
        assert (p.n_rg, p.n_cg) == (0, 0) and p.route == [SINGLE] * 64 and p.size == [(64, 48)] * 64
        p = Plan([req(w=-1, h=-1) for _ in range(32)] + [req(w=64, h=48) for _ in range(32)], enc, MIX_GPU)
        assert (p.n_rg, p.n_cg) == (0, 0) and p.route == [MIXED] * 64


def test_failed_decode_is_no_candidate():
    rs = [req(W=10 + k, H=10, w=5, h=5) for k in range(32)]  # 32 lone WebP requests
    assert Plan(rs, AUTO, MIX_GPU).route == [MIXED] * 32
    rs[7] = req(ok=0)
    p = Plan(rs, AUTO, MIX_GPU)  # 31 candidates: no mixed call
    assert not p.mixed and p.route == [SINGLE] * 7 + [NONE] + [SINGLE] * 24
    # nor a member of a group: 31 left of a geometry's 32
    rs = [req() for _ in range(32)]
    rs[0] = req(ok=0)
    p = Plan(rs, AUTO, MIX_HOST)
    assert p.route == [NONE] + [FRONT_GROUP] * 31 and p.rg[0] == -1


def test_sixteen_bit_is_neither_grouped_nor_a_candidate():
    p = Plan([req(), req(depth=2, pitch=512), req()], EXACT, MIX_GPU)
    assert p.rg == [0, -1, 0] and p.route == [EXACT_GROUP, SINGLE, EXACT_GROUP]
    p = Plan([req(W=10 + k, H=10, w=5, h=5) for k in range(31)] + [req(depth=2)], AUTO, MIX_GPU)
    assert not p.mixed  # 31 candidates
    p = Plan([req(depth=2), req(depth=2)], EXACT, MIX_GPU)
    assert not p.mixed and p.n_rg == 0 and p.route == [SINGLE, SINGLE]


def test_group_key_splits():
    for odd in (req(pitch=512), req(C=4), req(device=1), req(W=65), req(H=49), req(w=20, h=15)):
        p = Plan([req(), odd, req()], EXACT, MIX_HOST)
        assert p.rg == [0, -1, 0] and p.route == [EXACT_GROUP, SINGLE, EXACT_GROUP]


def test_oversize_webp_group_goes_to_the_per_image_error():
    big = dict(W=32768, H=16, pitch=98304, w=16384, h=8)
    for mix in (MIX_HOST, MIX_GPU):
        p = Plan([req(**big), req(**big)], EXACT, mix)
        assert p.size == [(16384, 8)] * 2 and p.rg == [0, 0]
        assert p.route == [SINGLE, SINGLE] and p.n_cg == 0  # encode_image_front reports the dimensions
    assert Plan([req(**big), req(**big)], EXACT, MIX_GPU).mixed  # counted, but not kept
    # at the limit itself the group is exact
    ok = dict(W=32766, H=16, pitch=98304, w=16383, h=8)
    assert Plan([req(**ok), req(**ok)], EXACT, MIX_HOST).route == [EXACT_GROUP] * 2


def test_a_target_resize_target_rejects():
    # a requested dimension above u32: "dimension exceeds u32" from the per-image ik_resize
    p = Plan([req(w=1 << 32, h=-1), req(w=1 << 32, h=-1), req(w=-1, h=1 << 40)], EXACT, MIX_GPU)
    assert p.route == [SINGLE] * 3 and p.n_rg == 0 and p.size == [(0, 0)] * 3
    assert p.mixed  # candidates all the same: the executor finds fewer than mixed_min kept


def test_resize_target_arithmetic():
    # one option None: the other scales it (f32, rounded), then the aspect fit (f64, rounded, at least 1)
    p = Plan([req(W=640, H=480, w=320, h=-1), req(W=640, H=480, w=-1, h=100), req(W=1000, H=10, w=10, h=10),
              req(W=3, H=2, w=1000, h=1)], LIBWEBP, MIX_HOST)
    assert p.size == [(320, 240), (133, 100), (10, 1), (2, 1)]


def mix40():
    rs = []
    rs += [req(q=80) for _ in range(9)] + [req(q=50) for _ in range(3)] + [req(fmt=JPEG, q=85) for _ in range(4)]
    rs += [req(fmt=AVIF, q=60) for _ in range(2)] + [req(fmt=JPEG, q=70)]
    rs += [req(W=100, H=80, pitch=512, w=50, h=-1, q=75) for _ in range(5)]
    rs += [req(W=100, H=80, pitch=512, w=25, h=20, fmt=JPEG, q=90) for _ in range(2)]
    rs += [req(C=4, q=80) for _ in range(3)] + [req(device=1, q=80) for _ in range(2)]
    rs += [req(w=-1, h=-1), req(w=64, h=48), req(depth=2, pitch=512), req(ok=0), req(ok=0, fmt=JPEG)]
    rs += [req(W=32768, H=16, pitch=98304, w=16384, h=8) for _ in range(2)]
    rs += [req(w=1 << 32, h=-1), req(W=7, H=5, w=3, h=3)]
    assert len(rs) == 40
    return rs


def test_request_order_does_not_change_the_plan():
    rs = mix40()
    rng = random.Random(20240)
    for enc, mix in ((AUTO, MIX_HOST), (EXACT, MIX_GPU), (EXACT, MIX_HOST), (LIBWEBP, MIX_GPU)):
        base = Plan(rs, enc, mix)
        perm = list(range(40))
        rng.shuffle(perm)  # shuffled[j] = rs[perm[j]]
        sh = Plan([rs[i] for i in perm], enc, mix)
        assert (sh.mixed, sh.mixed_min, sh.n_rg, sh.n_cg) == (base.mixed, base.mixed_min, base.n_rg, base.n_cg)
        back = lambda groups: [tuple(sorted(perm[j] for j in g)) for g in groups]  # noqa: E731
        rgs, cgs, route, size = sh.partition()
        brgs, bcgs, broute, bsize = base.partition()
        assert back(rgs) == brgs and back(cgs) == bcgs  # the same groups, in the same order
        for j, i in enumerate(perm):
            assert (route[j], size[j]) == (broute[i], bsize[i])
    # what that mix routes to under EXACT with the mixed call on
    p = Plan(rs, EXACT, MIX_GPU)
    assert p.mixed and p.n_rg == 6
    assert p.route[:19] == [EXACT_GROUP] * 12 + [JPEG_GROUP] * 4 + [SINGLE] * 3
    assert p.route[19:26] == [EXACT_GROUP] * 5 + [JPEG_GROUP] * 2
    assert p.route[26:31] == [EXACT_GROUP] * 5
    assert p.route[31:] == [MIXED, MIXED, SINGLE, NONE, NONE, SINGLE, SINGLE, SINGLE, MIXED]


def test_empty_batch():
    p = Plan([], AUTO, MIX_GPU)
    assert (p.mixed, p.n_rg, p.n_cg) == (False, 0, 0)
