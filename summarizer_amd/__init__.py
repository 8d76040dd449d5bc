"""summarizer_amd -- MI355X-native (gfx950) frame-importance scoring engine.

Host-side mirror of the reference's `summarizer/models/` scorer interface (VASNet, DSN, sLSTM and their
Trainers) over hand-written HIP kernels reached through the C ABI in include/sumk.h (libsumk.so, ctypes).
PyTorch is used for device memory, streams, autograd plumbing and torch.distributed only.
"""
__version__ = "0.1.0"

# Reference dotted path -> module of this package that replaces it.  Only the hot-path modules are
# aliased: `summarizer.utils.config / io` and `main.py` stay the reference's.  SumGAN-Att and the two baselines (logistic regression,
# random scores) are opt-in (OPT_IN_ALIASES, e.g. `install_as_reference(opt_in=("logistic", "random"))`): by default the reference's
# own modules run.
REFERENCE_ALIASES = {
    "summarizer.models.vasnet": "summarizer_amd.models.vasnet",            # VASNet, VASNetTrainer
    "summarizer.models.dsn": "summarizer_amd.models.dsn",                  # DSN, DSNTrainer
    "summarizer.models.sumgan": "summarizer_amd.models.sumgan",            # sLSTM ... SumGAN, SumGANTrainer
    "summarizer.models.transformer": "summarizer_amd.models.transformer",  # Transformer, TransformerTrainer
    "summarizer.utils.eval": "summarizer_amd.utils.eval",                  # upsample, generate_summary, evaluate_*
    "summarizer.utils.knapsack": "summarizer_amd.utils.knapsack",          # knapsack_ortools (native DP, no OR-tools)
}
OPT_IN_ALIASES = {
    "sumgan_att": ("summarizer.models.sumgan_att", "summarizer_amd.models.sumgan_att"),   # SumGANAtt, SumGANAttTrainer
    "logistic": ("summarizer.models.logistic", "summarizer_amd.models.logistic"),         # LogisticRegression, LogisticRegressionTrainer
    "random": ("summarizer.models.rand", "summarizer_amd.models.rand"),                   # Random, RandomTrainer
}


__all__ = ["Summarizer", "install_as_reference", "REFERENCE_ALIASES", "OPT_IN_ALIASES"]


def __getattr__(name):
    # `from summarizer_amd import Summarizer` (features in, summary out: summarize.py); resolved on first use so that importing the
    # package stays free of torch
    if name == "Summarizer":
        from .summarize import Summarizer
        return Summarizer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def install_as_reference(opt_in=()):
    """Make the reference's OWN files run on the HIP path without editing them: after this call
    `from summarizer.models.vasnet import VASNetTrainer` (summarizer/utils/config.py:12-18) -- and the same for dsn, sumgan,
    transformer, utils.eval, utils.knapsack -- resolve to this package, so `summarizer/utils/config.py` (HParameters, the
    `-m vasnet|dsn|sumgan|transformer` registry, config.py:68-77), `summarizer/main.py` and `benchmark.py` work unchanged.
    Call it before anything imports `summarizer.utils.config`; idempotent.  `opt_in` names further aliases of OPT_IN_ALIASES
    (e.g. ("sumgan_att",) or ("logistic", "random")).  Returns the list of installed aliases."""
    import importlib
    import sys
    unknown = [k for k in opt_in if k not in OPT_IN_ALIASES]
    if unknown:
        raise ValueError(f"unknown opt-in alias {unknown}; known: {sorted(OPT_IN_ALIASES)}")
    done = []
    for ref_name, own_name in list(REFERENCE_ALIASES.items()) + [OPT_IN_ALIASES[k] for k in opt_in]:
        mod = importlib.import_module(own_name)
        have = sys.modules.get(ref_name)
        if have is not None and have is not mod:
            raise ImportError(f"{ref_name} is already imported from {getattr(have, '__file__', '?')}: call "
                              "summarizer_amd.install_as_reference() before importing summarizer.utils.config / summarizer.main")
        sys.modules[ref_name] = mod
        done.append(ref_name)
    return done
