"""Device-backed mirror of sygnals/core/audio: features and the effects package."""
