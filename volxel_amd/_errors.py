"""The renderer's error type, apart from the renderer so that every part of it can raise it."""


class VolxelError(RuntimeError):
    """What viewer.ts:797-816 handleError receives."""
