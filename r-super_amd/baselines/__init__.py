"""Baselines R-Super is compared against (rsuper_train/baselines of the reference)."""
