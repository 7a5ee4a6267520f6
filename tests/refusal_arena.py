"""Device buffers for the refusal tests of the entries that compare byte ranges.  They are carved from ONE allocation, a
fixed distance apart, so that which buffers a displaced pointer meets -- and with that which refusal an entry words -- does
not depend on where the allocator happens to put separate tensors."""
import numpy as np

GAP = 1 << 15           # from one buffer's start to the next
LARGEST = GAP // 2      # a buffer's size: at least 16 KiB of nothing follow it, more than any test displaces a pointer


class Arena:
    def __init__(self, slots):
        import torch
        self.flat = torch.zeros((slots + 2) * GAP, dtype=torch.uint8, device="cuda")
        self.next = 1       # slot 0 and the last stay empty: pointers are displaced to either side

    def take(self, shape, dtype=None, fill=0):
        """A contiguous tensor of the given shape (uint8 unless dtype says otherwise), filled."""
        import torch
        dtype = dtype or torch.uint8
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        assert nbytes <= LARGEST and (self.next + 1) * GAP < self.flat.numel()
        t = self.flat[self.next * GAP:self.next * GAP + nbytes].view(dtype).view(tuple(shape))
        self.next += 1
        t.fill_(fill)
        return t

    def put(self, a):
        """A contiguous tensor holding the numpy array a."""
        import torch
        a = np.ascontiguousarray(a)
        t = self.take(a.shape, torch.from_numpy(a).dtype)
        t.copy_(torch.from_numpy(a))
        return t
