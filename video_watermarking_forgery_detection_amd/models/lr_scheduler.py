"""MultiStepLR_Restart and CosineAnnealingLR_Restart -- the learning-rate schedules of the reference's models/lr_scheduler.py:8-62 (which
every option file selects with train.lr_scheme and its models build per optimiser, IRNrhi_model.py:341-360), written against `param_groups`
directly: the optimisers here (optim.FlatAdam and its one-module form glayers.FlatAdamW) are flat-buffer objects, no torch.optim.Optimizer, so
torch's scheduler base cannot wrap them.  Any object with `param_groups` (a list of dicts with 'lr') works, torch's optimisers included.

What torch's base class does for the reference is reproduced by `_Schedule`: 'initial_lr' is set in every group at last_epoch == -1 and
required otherwise, base_lrs are the initial rates, and construction performs the first step() (last_epoch becomes 0).  The rates are
Python floats computed by the reference's recurrences in its order of operations -- lr * gamma ** count, the chained cosine
    (1 + cos(pi t / T)) / (1 + cos(pi (t - 1) / T)) * (lr - eta_min) + eta_min
and its (t - 1 - T) % (2 T) == 0 branch -- so a sequence equals the reference's bit for bit (tests/golden/lr_schedule.npz).

clear_state (MultiStep only, as in the reference): at a restart the optimiser's Adam state starts again from zero moments and step 0.  An
optimiser with `reset_state()` is asked to do that (the flat optimisers: on the device, in stream order, no host synchronisation); any
other gets the reference's `optimizer.state = defaultdict(dict)`.
"""
import math
from collections import Counter, defaultdict


class _Schedule:
    def __init__(self, optimizer, last_epoch=-1):
        self.optimizer = optimizer
        groups = optimizer.param_groups
        if last_epoch == -1:
            for g in groups:
                g.setdefault('initial_lr', g['lr'])
        else:
            for i, g in enumerate(groups):
                if 'initial_lr' not in g:
                    raise KeyError("param 'initial_lr' is not specified in param_groups[{}] when resuming an optimizer".format(i))
        self.base_lrs = [g['initial_lr'] for g in groups]
        self.last_epoch = last_epoch
        self.step()

    def get_lr(self):
        raise NotImplementedError

    def step(self):
        self.last_epoch += 1
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g['lr'] = lr
        self._last_lr = [g['lr'] for g in self.optimizer.param_groups]

    def get_last_lr(self):
        return self._last_lr

    def state_dict(self):
        """everything but the optimiser (whose own state_dict carries 'lr' and 'initial_lr')"""
        return {k: v for k, v in self.__dict__.items() if k != 'optimizer'}

    def load_state_dict(self, state_dict):
        self.__dict__.update(state_dict)

    def _restart_weight(self):
        return self.restart_weights[self.restarts.index(self.last_epoch)]


class MultiStepLR_Restart(_Schedule):
    def __init__(self, optimizer, milestones, restarts=None, weights=None, gamma=0.1, clear_state=False, last_epoch=-1):
        self.milestones = Counter(milestones)   # a milestone listed twice applies gamma twice
        self.gamma = gamma
        self.clear_state = clear_state
        self.restarts = restarts if restarts else [0]
        self.restart_weights = weights if weights else [1]
        assert len(self.restarts) == len(self.restart_weights), 'restarts and their weights do not match.'
        super().__init__(optimizer, last_epoch)

    def _clear(self):
        reset = getattr(self.optimizer, 'reset_state', None)
        if reset is not None:
            reset()
        else:
            self.optimizer.state = defaultdict(dict)

    def get_lr(self):
        groups, t = self.optimizer.param_groups, self.last_epoch
        if t in self.restarts:    # (a restart wins over a milestone at the same step)
            if self.clear_state:
                self._clear()
            w = self._restart_weight()
            return [g['initial_lr'] * w for g in groups]
        if t not in self.milestones:
            return [g['lr'] for g in groups]
        return [g['lr'] * self.gamma ** self.milestones[t] for g in groups]


class CosineAnnealingLR_Restart(_Schedule):
    def __init__(self, optimizer, T_period, restarts=None, weights=None, eta_min=0, last_epoch=-1):
        self.T_period = T_period
        self.T_max = self.T_period[0]   # the current period
        self.eta_min = eta_min
        self.restarts = restarts if restarts else [0]
        self.restart_weights = weights if weights else [1]
        self.last_restart = 0
        assert len(self.restarts) == len(self.restart_weights), 'restarts and their weights do not match.'
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        groups, t = self.optimizer.param_groups, self.last_epoch
        if t == 0:
            return self.base_lrs
        if t in self.restarts:
            self.last_restart = t
            self.T_max = self.T_period[self.restarts.index(t) + 1]
            w = self._restart_weight()
            return [g['initial_lr'] * w for g in groups]
        T, since = self.T_max, t - self.last_restart
        if (since - 1 - T) % (2 * T) == 0:   # the first step up from eta_min: the chained quotient below would divide by 1 + cos(pi) = 0
            return [g['lr'] + (base - self.eta_min) * (1 - math.cos(math.pi / T)) / 2 for base, g in zip(self.base_lrs, groups)]
        return [(1 + math.cos(math.pi * since / T)) / (1 + math.cos(math.pi * (since - 1) / T)) * (g['lr'] - self.eta_min) + self.eta_min
                for g in groups]


def build_schedulers(optimizers, train_opt):
    """one scheduler per optimiser from the reference's train.* keys (IRNrhi_model.py:341-356): lr_scheme = 'MultiStepLR' (lr_steps,
    lr_gamma, restarts, restart_weights, clear_state) | 'CosineAnnealingLR_Restart' (T_period, eta_min, restarts, restart_weights); no
    lr_scheme: no scheduler, the learning rate stays where the optimiser has it; any other value raises as the reference does"""
    get = (lambda k, default=None: default if train_opt is None or train_opt.get(k) is None else train_opt.get(k))
    scheme = get('lr_scheme')
    if scheme is None:
        return []
    if scheme == 'MultiStepLR':
        return [MultiStepLR_Restart(o, list(get('lr_steps', [])), restarts=get('restarts'), weights=get('restart_weights'),
                                    gamma=get('lr_gamma', 0.1), clear_state=bool(get('clear_state', False))) for o in optimizers]
    if scheme == 'CosineAnnealingLR_Restart':
        return [CosineAnnealingLR_Restart(o, get('T_period'), eta_min=get('eta_min', 0), restarts=get('restarts'),
                                          weights=get('restart_weights')) for o in optimizers]
    raise NotImplementedError('MultiStepLR learning rate scheme is enough.')
