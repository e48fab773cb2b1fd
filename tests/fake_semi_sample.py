"""TEST INFRASTRUCTURE ONLY -- NumPy executable specification of t3d_semi_sample (include/t3d.h, csrc/data.hip k_semi_sample), on host
pointers, so that the drivers' SEMI_SAMPLING_METHOD paths run end to end through Runtime(device='cpu', lib=FakeSemiLib()).  The draws
come from the same counter-based hash as the kernel's, in uint64 / float32 NumPy arithmetic: device and specification agree exactly
on `sample` and `is_data_2D`."""
import numpy as np

from fake_t3d import AbiSizeError, FakeLib, _struct, arr
from transferable3d_amd import abi

M64 = (1 << 64) - 1
ERR_ARG, ERR_SHAPE = -1, -2


def mix_u32(x):
    """csrc/data.hip mix_u32 on a Python int."""
    x &= M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return (x >> 16) & 0xffffffff


def u01(r):
    return (np.float32(r >> 8) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def step_key(seed, step):
    return ((((seed & 0xffffffff) << 32) ^ ((step * 0x9E3779B97F4A7C15) & M64)) + 0x8CB92BA72F3D8DD7) & M64


def coin(seed, step, equal_prob):
    """The step's coin: equal classes when true."""
    return bool(u01(mix_u32(step_key(seed, step) + 7)) < np.float32(equal_prob))


def half_key(seed, step, from2d):
    return (step_key(seed, step) + (1 if from2d else 2) * 0x94D049BB133111EB) & M64


def group_sizes(hk, n, k):
    """Slots per class: base + 1 for the classes whose key ranks among the n % k smallest (ties: lower index first)."""
    keys = [u01(mix_u32(hk + (i + 1) * 0xA24BAED4963EE407)) for i in range(k)]
    rank = [sum(1 for j in range(k) if keys[j] < keys[i] or (keys[j] == keys[i] and j < i)) for i in range(k)]
    return [n // k + (1 if rank[i] < n % k else 0) for i in range(k)]


def draw(lst, n, seed, step, from2d, equal):
    """n slots from one list: lst = dict(ids, members, offsets, n_groups) of host arrays.  Returns the frustum ids."""
    hk = half_key(seed, step, from2d)
    out = np.zeros(n, np.int32)
    if equal:
        k, off = lst['n_groups'], lst['offsets']
        b = 0
        for i, size in enumerate(group_sizes(hk, n, k)):
            lo, ln = int(off[i]), int(off[i + 1] - off[i])
            for _ in range(size):
                u = u01(mix_u32(hk + (b + 1) * 0xD6E8FEB86659FD93))
                out[b] = lst['members'][lo + min(int(u * np.float32(ln)), ln - 1)]
                b += 1
        return out
    ln, moved = len(lst['ids']), {}
    for i in range(n):                        # partial Fisher-Yates over the virtual array 0..len-1
        t = i + ((mix_u32(hk + (i + 1) * 0xC2B2AE3D27D4EB4F) * max(ln - i, 1)) >> 32)
        vi, vt = moved.get(i, i), moved.get(t, t)
        out[i] = lst['ids'][min(vt, ln - 1)]
        moved[t] = vi
    return out


def semi_sample_spec(method, list3d, list2d, B, seed, step, equal_prob=0.0, perm=None, perm_len=0):
    """(sample [B], is_data_2D [B]) of step `step`.  method: abi.SEMI_*; the lists as in `draw`; perm: BATCH's epoch permutation."""
    sample, flag = np.zeros(B, np.int32), np.zeros(B, np.int32)
    if method == abi.SEMI_BATCH:
        n3, total = len(list3d['ids']), len(list3d['ids']) + len(list2d['ids'])
        for b in range(B):
            e = min(max(int(perm[(step * B + b) % perm_len]), 0), total - 1)
            flag[b] = 1 if e >= n3 else 0
            sample[b] = list2d['ids'][e - n3] if e >= n3 else list3d['ids'][e]
        return sample, flag
    equal = coin(seed, step, equal_prob)
    if method == abi.SEMI_ALTERNATE_BATCH:
        from2d = step % 2 == 0
        sample[:] = draw(list2d if from2d else list3d, B, seed, step, from2d, equal)
        flag[:] = 1 if from2d else 0
    else:
        h = B // 2
        sample[:h], flag[:h] = draw(list2d, h, seed, step, True, equal), 1
        sample[h:], flag[h:] = draw(list3d, h, seed, step, False, equal), 0
    return sample, flag


def host_list(g):
    """A t3d_semi_list of host pointers -> dict of arrays."""
    n = g.n_groups
    off = arr(g.offsets, n + 1) if n > 0 and g.offsets else None
    return dict(ids=arr(g.ids, g.len) if g.len > 0 and g.ids else np.zeros(0, np.int32),
                members=arr(g.members, g.len) if n > 0 and g.members else None, offsets=off, n_groups=n)


class FakeSemiLib(FakeLib):
    def t3d_semi_sample(self, a, stream):
        """The launcher's checks in the launcher's order, then the kernel."""
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if not p.hyper or not p.sample or not p.is_data_2D:
            return ERR_ARG
        B = p.B
        if B <= 0 or B > abi.SEMI_SAMPLE_MAX_B:
            return ERR_SHAPE
        if p.method == abi.SEMI_BATCH:
            if not p.perm or p.perm_len <= 0 or p.list3d.len < 0 or p.list2d.len < 0 or p.list3d.len + p.list2d.len <= 0:
                return ERR_ARG
            if (p.list3d.len > 0 and not p.list3d.ids) or (p.list2d.len > 0 and not p.list2d.ids):
                return ERR_ARG
        elif p.method in (abi.SEMI_ALTERNATE_BATCH, abi.SEMI_MIXED_BATCH):
            mixed = p.method == abi.SEMI_MIXED_BATCH
            if mixed and B % 2:
                return ERR_SHAPE
            n = B // 2 if mixed else B
            for g in (p.list3d, p.list2d):
                if g.len <= 0 or not g.ids:
                    return ERR_ARG
                if g.n_groups < 0 or g.n_groups > 32:
                    return ERR_SHAPE
                if p.equal_prob > 0.0 and (g.n_groups == 0 or not g.members or not g.offsets):
                    return ERR_ARG
                if p.equal_prob < 1.0 and g.len < n:
                    return ERR_SHAPE
        else:
            return ERR_ARG
        step = int(arr(p.hyper, 1)[0])
        perm = arr(p.perm, p.perm_len) if p.method == abi.SEMI_BATCH else None
        sample, flag = semi_sample_spec(p.method, host_list(p.list3d), host_list(p.list2d), B, p.seed, step, p.equal_prob, perm, p.perm_len)
        arr(p.sample, B)[:] = sample
        arr(p.is_data_2D, B)[:] = flag
        return 0
