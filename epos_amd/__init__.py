"""EPOS inference hot path on MI355X."""
