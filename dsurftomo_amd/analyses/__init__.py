"""The optional analyses of the inversion loop (invert.py), one module each; common.py states what a module defines."""
