"""Samplers behind stochopy's ``sample`` API: Metropolis-Hastings and Hamiltonian Monte-Carlo with many independent,
device-resident chains (reference: stochopy/sample)."""
from ._ensemble import sample as ensemble
from ._helpers import SampleResult, sample
from ._hmc import sample as hmc
from ._mcmc import sample as mcmc
from ._smc import sample as smc

__all__ = [
    "SampleResult",
    "sample",
    "ensemble",
    "hmc",
    "mcmc",
    "smc",
]
