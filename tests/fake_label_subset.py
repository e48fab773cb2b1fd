"""TEST INFRASTRUCTURE ONLY -- NumPy executable specification of t3d_label_subset (include/t3d.h, csrc/data.hip k_label_subset), on host
pointers: the lists and class groups of a data set object, from membership flags or from two hash draws per frustum.  The draws come
from the same counter-based hash as the kernel's (fake_semi_sample.mix_u32 / u01), in uint64 / float32 arithmetic: device and
specification agree exactly on every output."""
import numpy as np

from fake_semi_sample import M64, FakeSemiLib, mix_u32, u01
from fake_t3d import AbiSizeError, _struct, arr
from transferable3d_amd import abi

ERR_ARG, ERR_SHAPE = -1, -2
NUM_CLASS = abi.NUM_CLASS


def hash_selected(cls, class_mask, keep_prob, add_prob, seed):
    """member == NULL: frustum f is selected iff (class_mask[cls[f]] and u1 <= keep_prob) or u2 < add_prob."""
    key = (((seed & 0xffffffff) << 32) + 0x3C79AC492BA7B653) & M64
    keep, add = np.float32(keep_prob), np.float32(add_prob)
    out = np.zeros(len(cls), bool)
    for f, c in enumerate(cls):
        u1 = u01(mix_u32(key + (2 * f + 1) * 0xA24BAED4963EE407))
        u2 = u01(mix_u32(key + (2 * f + 2) * 0xA24BAED4963EE407))
        out[f] = bool((class_mask[c] != 0 and u1 <= keep) or u2 < add)
    return out


def label_subset_spec(cls, member=None, class_mask=None, keep_prob=1.0, add_prob=-1.0, seed=20):
    """dict(ids [F], members [F], offsets [NUM_CLASS + 1], present [NUM_CLASS], len, n_groups) as the kernel writes them."""
    cls = np.asarray(cls, np.int32)
    F = len(cls)
    sel = np.asarray(member).astype(bool) if member is not None else hash_selected(cls, class_mask, keep_prob, add_prob, seed)
    ids = np.nonzero(sel)[0].astype(np.int32)
    n = len(ids)
    present = np.array([int((cls[ids] == c).any()) for c in range(NUM_CLASS)], np.int32)
    groups = [ids[cls[ids] == c] for c in range(NUM_CLASS) if present[c]]
    offsets = np.full(NUM_CLASS + 1, n, np.int32)
    offsets[:len(groups) + 1] = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    pad = lambda v: np.concatenate([v, np.full(F - len(v), -1)]).astype(np.int32)
    return dict(ids=pad(ids), members=pad(np.concatenate(groups) if groups else np.zeros(0, np.int32)), offsets=offsets, present=present,
                len=n, n_groups=len(groups))


class FakeLabelLib(FakeSemiLib):
    def t3d_label_subset(self, a, stream):
        """The launcher's checks in the launcher's order, then the kernel."""
        try:
            p = _struct(a)
        except AbiSizeError:
            return abi.ERR_ABI
        if not p.cls or not p.ids or not p.members or not p.offsets or not p.present or not p.summary:
            return ERR_ARG
        if not p.member and not p.class_mask:
            return ERR_ARG
        F = p.F
        if F <= 0:
            return ERR_SHAPE
        cls = arr(p.cls, F)
        bad = bool(((cls < 0) | (cls >= NUM_CLASS)).any())
        if bad:              # such a data set selects nothing
            s = label_subset_spec(np.zeros(F, np.int32), member=np.zeros(F, np.uint8))
        else:
            member = np.ctypeslib.as_array(p.member, shape=(F,)) if p.member else None
            s = label_subset_spec(cls, member, arr(p.class_mask, NUM_CLASS) if p.class_mask else None, p.keep_prob, p.add_prob, p.seed)
        arr(p.ids, F)[:], arr(p.members, F)[:] = s['ids'], s['members']
        arr(p.offsets, NUM_CLASS + 1)[:], arr(p.present, NUM_CLASS)[:] = s['offsets'], s['present']
        arr(p.summary, 4)[:] = [s['len'], s['n_groups'], int(bad), 0]
        return ERR_ARG if bad else 0
