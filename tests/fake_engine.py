"""The stand-in the CPU tests hand to checkpoint.save_training_checkpoint / resume_training in place of a TrainEngine (the engine
itself needs the GPU).  tests/test_gpu_engine_options.py ties it to the real classes: their attributes carry the same names."""
import torch


class FakeEngine(object):
    """What the checkpoint code uses of a TrainEngine.  options: values of spec.MODEL_OPTIONS rows by keyword; only those given
    become attributes (an engine without an attribute means the row's default)."""

    def __init__(self, sd, **options):
        self.sd, self.opt_state = dict(sd), None
        vars(self).update(options)

    def state_dict(self):
        return dict(self.sd)

    def optimizer_state_dict(self):
        return {"momentum_buffer": {k: torch.zeros_like(v) for k, v in self.sd.items()}, "steps": 3, "lr": 0.01,
                "momentum": 0.9, "weight_decay": 1e-4}

    def load_optimizer_state_dict(self, st):
        self.opt_state = st
