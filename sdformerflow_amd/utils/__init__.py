"""The reference's `utils` package, as far as this package builds it: visualization (stored results) and its PNG codec."""
