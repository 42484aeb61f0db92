"""The reference's learning-rate schedule (solver/lr_scheduler.py:10-52, WarmupMultiStepLR; built by solver/build.py:29-37 from
SOLVER.*), as a function of the update's index.  Host code: TrainEngine(lr_schedule=...) asks it for the rate of every step,
checkpoint.save_training_checkpoint / resume_training store and compare it."""
from bisect import bisect_right

# config/defaults.py:433-446 (SOLVER.BASE_LR, STEPS, GAMMA, WARMUP_FACTOR, WARMUP_ITERS, WARMUP_METHOD, BIAS_LR_FACTOR)
BASE_LR, STEPS, GAMMA, WARMUP_FACTOR, WARMUP_ITERS, WARMUP_METHOD, BIAS_LR_FACTOR = 0.001, (30000,), 0.1, 1.0 / 3, 500, "linear", 2
_FIELDS = ("milestones", "gamma", "warmup_factor", "warmup_iters", "warmup_method", "base_lrs")      # state_dict() less last_epoch


class LRSchedule(object):
    """WarmupMultiStepLR.get_lr as lr_at(k): the rate of the k-th update, k = 0, 1, ...

    The reference calls scheduler.step() AFTER optimizer.step() (engine/trainer.py:93-96), and the scheduler's constructor leaves
    last_epoch at 0: update k runs at the rate get_lr() gives for last_epoch == k.  The arithmetic is the reference's, in its order
    (base_lr * warmup_factor * gamma ** bisect_right(milestones, k), lr_scheduler.py:40-52), so the double is bit-equal to what the
    reference writes into its first parameter group; the second group (biases, solver/build.py:8-26) runs at BIAS_LR_FACTOR = 2
    times that, which the update kernels form from a table entry's lr_mult."""

    def __init__(self, base_lr=BASE_LR, milestones=STEPS, gamma=GAMMA, warmup_factor=WARMUP_FACTOR, warmup_iters=WARMUP_ITERS,
                 warmup_method=WARMUP_METHOD):
        if not list(milestones) == sorted(milestones):                                  # lr_scheduler.py:21-25
            raise ValueError("Milestones should be a list of increasing integers. Got %r" % (milestones,))
        if warmup_method not in ("constant", "linear"):                                 # lr_scheduler.py:27-31
            raise ValueError("Only 'constant' or 'linear' warmup_method accepted, got %r" % (warmup_method,))
        self.base_lr, self.milestones, self.gamma = base_lr, tuple(milestones), gamma
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method

    @classmethod
    def of_record(cls):
        """configs/fcos/2019_10_25_vanilla_siamse_backbone.yaml:50-58 over the defaults: 0.0005, held at the warmup factor 1/3 for 100
        iterations, divided by 10 at 60 000, 90 000 and 120 000."""
        return cls(base_lr=0.0005, milestones=(60000, 90000, 120000), warmup_iters=100, warmup_method="constant")

    def lr_at(self, k):
        warmup_factor = 1
        if k < self.warmup_iters:
            if self.warmup_method == "constant":
                warmup_factor = self.warmup_factor
            elif self.warmup_method == "linear":
                alpha = float(k) / self.warmup_iters
                warmup_factor = self.warmup_factor * (1 - alpha) + alpha
        return float(self.base_lr * warmup_factor * self.gamma ** bisect_right(self.milestones, k))

    def state_dict(self, last_epoch=0):
        """The reference scheduler's own attributes (utils/checkpoint.py:44-45 saves scheduler.state_dict() = its __dict__ less the
        optimizer): its class could load this with __dict__.update.  base_lrs: the two parameter groups' initial rates."""
        return {"milestones": list(self.milestones), "gamma": self.gamma, "warmup_factor": self.warmup_factor,
                "warmup_iters": self.warmup_iters, "warmup_method": self.warmup_method,
                "base_lrs": [self.base_lr, BIAS_LR_FACTOR * self.base_lr], "last_epoch": int(last_epoch)}

    def load_state_dict(self, state):
        """Take the schedule of a state_dict(); -> its last_epoch (the schedule itself has no position: lr_at takes one)."""
        new = LRSchedule(state["base_lrs"][0], state["milestones"], state["gamma"], state["warmup_factor"], state["warmup_iters"],
                         state["warmup_method"])
        vars(self).update(vars(new))
        return int(state.get("last_epoch", 0))

    def differences(self, state):
        """[(field, this schedule's value, the state's value)] over every field but last_epoch."""
        mine = self.state_dict()
        return [(f, mine[f], state.get(f)) for f in _FIELDS
                if (list(state[f]) if f in ("milestones", "base_lrs") and f in state else state.get(f)) != mine[f]]
