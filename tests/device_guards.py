"""What the tests that call the C ABI on slices of larger device buffers share: a byte buffer with guard bytes in front of and
behind the slice a kernel is given, the check that the kernel left them alone, and the return-code check of a raw call."""


def guarded(n_bytes, lead, trail, fill):
    """a device buffer of `fill` bytes and the view of n_bytes that starts `lead` bytes into it"""
    import torch
    buf = torch.full((lead + n_bytes + trail,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + n_bytes]


def guards_kept(buf, lead, n_bytes, fill):
    """the bytes in front of and behind the view still hold `fill`"""
    b = buf.cpu().numpy()
    return bool((b[:lead] == fill).all() and (b[lead + n_bytes:] == fill).all())


def ok(native, rc):
    native.check(rc)
