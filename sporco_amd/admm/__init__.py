"""Solver classes mirroring the reference sub-package of the same name."""

__all__ = ['admm', 'bpdn', 'cbpdn', 'cbpdn_cplx', 'cbpdnin', 'cbpdntv', 'ccmod', 'ccmodmd', 'cmod', 'pdcsc', 'rpca', 'spline', 'tvl1', 'tvl2']
