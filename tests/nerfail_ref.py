"""numpy restatement of the DeepFool gate, of the choice inside the DeepFool step and of the pass bookkeeping of the NeRFail loop,
written from include/nerfail_hip.h (DeepFool gate and step) and the reference's attack_NeRFail.py (= AN) / deepfool.py (= DF),
not from the kernels. Used by the CPU test against fixture g27 and by the GPU tests of the two entry points."""
import numpy as np

MAX_COMPETITORS = 8


def gate(cla, o, target, m1, m2, dtype=np.float32):
    """DF:53-66 and the f' of DF:79 / :93. `cla`: the C logits; target: -1 untargeted. Returns the record as a dict:
    done, argmax (-1 with a NaN in the bumped row), n_comp, targeted, cls [8], fabs [8]."""
    cla = np.asarray(cla, dtype).reshape(-1)
    C = cla.shape[0]
    m1, m2 = dtype(m1), dtype(m2)
    b = cla.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        if target < 0:
            b[o] = b[o] + m1
        else:
            for c in range(C):
                if c != target:
                    b[c] = b[c] + m1
    if np.isnan(b).any():
        arg = -1
    else:
        arg = int(np.argmax(b))                                          # numpy's argmax is the first maximum
    done = arg >= 0 and (arg != o if target < 0 else arg == target)
    ks = [k for k in range(C) if k != o] if target < 0 else [target]
    cls = np.full(MAX_COMPETITORS, -1, np.int32)
    fabs = np.zeros(MAX_COMPETITORS, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        for r, k in enumerate(ks):
            cls[r] = k
            fabs[r] = np.abs(dtype(b[k] - dtype(b[o] + m2)))
    return dict(done=int(done), argmax=arg, n_comp=len(ks), targeted=int(target >= 0), cls=cls, fabs=fabs, bumped=b)


def record_words(rec):
    """The record as the 20 32-bit words of struct nerfail_deepfool_record."""
    return np.concatenate([np.array([rec['done'], rec['argmax'], rec['n_comp'], rec['targeted']], np.int32), rec['cls'].astype(np.int32),
                           rec['fabs'].astype(np.float32).view(np.int32)])


def choose(fabs, norms2, n_comp, targeted, K=None, dtype=np.float32):
    """DF:81-96 in `dtype`, one rounding per operation: (slice 1..K of the gradients or 1 when nothing was chosen, scale,
    competitor index or -1). K = n_rhs - 1 of the call; a record whose n_comp is not K chooses nothing."""
    K = n_comp if K is None else K
    if n_comp != K:
        return 1, dtype(0), -1
    fabs, norms2 = np.asarray(fabs, dtype), np.asarray(norms2, dtype)
    eps = dtype(0.0001)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if targeted:
            nrm = np.sqrt(norms2[0])
            return 1, dtype(fabs[0] / dtype(dtype(nrm * nrm) + eps)), 0
        minv, bi = dtype(np.inf), -1
        for r in range(K):
            v = dtype(fabs[r] / dtype(np.sqrt(norms2[r]) + eps))
            if np.isnan(v):
                v = dtype(np.inf)
            if v < minv:
                minv, bi = v, r
        if bi < 0:
            return 1, dtype(0), -1
        nrm = np.sqrt(norms2[bi])
        return bi + 1, dtype(fabs[bi] / dtype(dtype(nrm * nrm) + eps)), bi


class Book:
    """The host bookkeeping of AN:294-503 as a state machine: begin_pass, visit per DeepFool call, end_pass."""

    def __init__(self, epochs, m1, m2, targeted, df_max_iter, m2_max_limit=10000, accumulate_incomplete=False):
        self.epochs, self.m1, self.args_m2, self.targeted = epochs, m1, m2, targeted
        self.df_max_iter, self.limit, self.acc_inc = df_max_iter, m2_max_limit, accumulate_incomplete
        self.m1_list = [0, m1]
        self.best_acc = 0 if targeted else 10000
        self.m1_best = self.m2_best = 0
        self.epoch = 0

    def running(self):
        return self.epoch < self.epochs

    def begin_pass(self):
        self.no_attack = self.attack_all = 0
        self.m2 = self.args_m2                                            # AN:332
        self.not_changed = True
        self.raises = 0
        return self.epoch == self.epochs - 1                              # export pass

    def visit(self, iter_k):
        """One DeepFool call that returned iter_k (AN:405-418). Returns whether its perturbation is added to the table."""
        if iter_k < self.df_max_iter or self.acc_inc:
            self.not_changed = False
            self.attack_all += 1
            return True
        if self.m2 < self.limit:
            self.no_attack += 1
            self.attack_all += 1
            if self.attack_all > 10 and (self.no_attack / self.attack_all) > 0.5:
                self.m2 = self.m2 * 10
                self.raises += 1
                self.no_attack = self.attack_all = 0
        return False

    def exported(self):
        self.not_changed = False                                          # AN:432

    def end_pass(self, attack_acc):
        """AN:434-503: the m1 bisection, the epoch step, the best rule. Returns taken."""
        e, last = self.epoch, self.epochs - 1
        if self.not_changed:
            if self.m1_list[0] < self.m1 - 1 and e == 0:
                self.m1_list[1] = self.m1
                self.m1 = int((self.m1 + self.m1_list[0]) / 2)
                self.m2 = self.args_m2
                self.epoch = 0
            elif self.m1_list[0] < self.m1 and e == 0:
                self.m1_list[1] = self.m1
                self.m1 = self.m1_list[0]
                self.m2 = self.args_m2
                self.epoch = 0
            else:
                self.epoch = last
        elif e == last:
            if self.m1 < self.m1_list[1] - 1:
                self.m1_list[0] = self.m1
                self.m1 = int((self.m1 + self.m1_list[1]) / 2)
                self.m2 = self.args_m2
                self.epoch = 0
            elif self.m1 < self.m1_list[1]:
                self.m1_list[0] = self.m1
                self.m1 = self.m1_list[1]
                self.m2 = self.args_m2
                self.epoch = 0
            else:
                self.epoch += 1
        else:
            self.epoch += 1
        if self.targeted:
            take = (attack_acc >= self.best_acc and self.m1 == self.m1_best) or (self.m1 > self.m1_best and attack_acc > 0)
        else:
            take = (attack_acc <= self.best_acc and self.m1 == self.m1_best) or (self.m1 > self.m1_best and attack_acc < 1)
        if take:
            self.best_acc, self.m1_best, self.m2_best = attack_acc, self.m1, self.m2
        return bool(take)


def ce(logits, label):
    z = np.asarray(logits, np.float64)
    m = z.max(-1, keepdims=True)
    return (m[..., 0] + np.log(np.exp(z - m).sum(-1))) - z[..., label]
