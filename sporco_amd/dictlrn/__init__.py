"""Solver classes mirroring the reference sub-package of the same name."""

__all__ = ['bpdndl', 'cbpdndl', 'cbpdndlmd', 'common', 'dictlrn', 'onlinecdl', 'wbpdndl']
