"""The stream hand-off of every call that takes a `stream`: the one place where a raw HIP stream handle meets torch's streams."""


class Handoff:
    """A call runs on `stream` (a raw handle) or, with None, on torch's current stream of `where` (a device, or a tensor on it): `target`
    is that torch stream, `handle` its raw handle for the C call, `other` whether it is not the current stream.  The target first waits
    for the work queued so far on the current stream, which wrote the inputs."""

    def __init__(self, where, stream=None):
        import torch
        device = getattr(where, "device", where)
        self.current = torch.cuda.current_stream(device)
        self.target = self.current if stream is None else torch.cuda.ExternalStream(int(stream), device=device)
        self.handle = self.target.cuda_stream
        self.other = self.handle != self.current.cuda_stream
        if self.other:
            self.target.wait_stream(self.current)

    def on_target(self):
        """a context in which torch allocates from the target's pool, and issues its own work there"""
        import torch
        return torch.cuda.stream(self.target)

    def reads(self, *tensors):
        """mark tensors as in use on the target: the caching allocator must not hand their memory out again while the call still uses it"""
        if self.other:
            for t in tensors:
                t.record_stream(self.target)

    def join(self):
        """the current stream waits for the result"""
        if self.other:
            self.current.wait_stream(self.target)
