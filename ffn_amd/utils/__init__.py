"""Utilities around inference: preparation of agglomeration requests."""
