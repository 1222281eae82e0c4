"""The three no-LayerNorm models of tests/golden/residual_noln.npz (written from the reference by
tests/golden/make_golden_residual.py), each read as a fixture of its own so tests/golden_util's helpers
(config, prefixed, batch_from) take it."""
from tests.golden_util import config, load, prefixed

CASES = ("simple", "sample", "meta")


class Case:
    """The arrays stored under ``<case>/`` as ``d[key]`` / ``d.files`` / ``key in d``."""

    def __init__(self, d, case):
        self._d, self._p = d, case + "/"
        self.files = [k[len(self._p):] for k in d.files if k.startswith(self._p)]

    def __getitem__(self, key):
        return self._d[self._p + key]

    def __contains__(self, key):
        return key in self.files


def load_case(case):
    return Case(load("residual_noln"), case)


def model_class(case):
    from multimodalreactiongeneration_amd import model
    return {"simple": model.SimpleLSTM, "sample": model.LSTMwithSample, "meta": model.Metaformer}[case]


def build(case, device=None):
    """(model with the golden's parameters loaded strictly, fixture, config)."""
    d = load_case(case)
    cfg = config(d)
    m = model_class(case)(cfg["model"], cfg["optim"], cfg["metrics"])
    m.load_state_dict(prefixed(d, "param/"), strict=True)
    return (m if device is None else m.to(device)), d, cfg
