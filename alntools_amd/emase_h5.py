# -*- coding: utf-8 -*-
"""EMASE ``.h5`` container (``Sparse3DMatrix.save`` / ``AlignmentPropertyMatrix.save``,
``Sparse3DMatrix.py:325-342``, ``AlignmentPropertyMatrix.py:507-532``).

Logical layout: root attrs ``incidence_only``, ``mtype='csc_matrix'``, ``shape=(T, H, E)``; groups
``/h0../h{H-1}`` with uint32 ``indptr``/``indices`` (and float64 ``data`` unless incidence-only);
``/lengths`` (T x H); ``/count`` (vector, or group indptr/indices/data when 2-D); attr ``hname``;
arrays ``/lname``, ``/rname``, ``/sname``.

PyTables (the reference's writer) and h5py are both absent from this image; the fallback is a ctypes binding of
libhdf5 itself (``h5lite.py``), which writes the same groups, datasets (chunked, shuffle + deflate 1) and attributes
(tuples/lists pickled, as PyTables stores them).  The byte/attribute-level structure PyTables produces is NOT pinned by
any fixture ("parity unpinned: .h5"): what is tested is the logical round trip .bin -> .h5 -> .bin.
"""
from __future__ import annotations

import numpy as np


def _backend():
    try:
        import tables  # noqa: F401
        return "tables"
    except ImportError:
        pass
    try:
        import h5py  # noqa: F401
        return "h5py"
    except ImportError:
        pass
    from . import h5lite
    h5lite.lib()                       # raises with a clear message if libhdf5 is missing too
    return "libhdf5"


class _Csc(object):
    """indptr / indices / data of one haplotype's E x T incidence matrix, as ``apm.data[h]`` holds them after ``finalize()``."""

    def __init__(self, indptr, indices, data=None):
        self.indptr, self.indices = indptr, indices
        self.data = np.ones(len(indices), dtype=np.float64) if data is None else data


def _device(device=None):
    """Index of the GPU the conversions run on: the one named, else ``ALNTOOLS_GPU`` (default 0)."""
    import os
    return int(os.environ.get("ALNTOOLS_GPU", "0")) if device is None else int(device)


def device_hapcsc(m, device=None):
    """CSR(bitmask) A -> one CSC matrix per haplotype, on the GPU (``ecb_csr_to_hapcsc``: the sparse-format half of
    ``bin_utils.ec2emase`` / ``Sparse3DMatrix.finalize``, ``bin_utils.py:979-995``, ``Sparse3DMatrix.py:189-193``).
    Host arrays in, host arrays out -- libecb holds the device buffers itself, PyTorch is not involved.
    No CPU path: without a GPU this raises, like the rest of the hot path."""
    from . import ecb
    cptr, cidx = ecb.csr_to_hapcsc_host(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, _device(device))
    out, start = [], 0
    for h in range(m.num_haplotypes):
        n = int(cptr[h, -1])
        out.append(_Csc(cptr[h], cidx[start:start + n]))
        start += n
    return out


def split_hapcsc(cptr, cidx, cdata=None):
    """(csc_indptr [H, T+1], csc_indices [total], csc_data [total] or None) as libecb lays them out -> one :class:`_Csc` per haplotype."""
    out, start = [], 0
    for h in range(len(cptr)):
        n = int(cptr[h][-1])
        out.append(_Csc(cptr[h], cidx[start:start + n], None if cdata is None else cdata[start:start + n]))
        start += n
    return out


def device_hapcsc_values(values, device=None):
    """A ``hapcsc`` for :func:`save` whose matrices carry ``values`` -- float64, one per set bit of A in bit order (``ecb.posterior``'s
    ``post``) -- as their ``data``, transposed on the GPU (``ecb_csr_to_hapcsc_values``): with ``incidence_only=False`` the file then holds
    the posterior, zeros included, where ``ec2emase`` writes ones.  Indptr and indices are :func:`device_hapcsc`'s."""
    def convert(m):
        from . import ecb
        return split_hapcsc(*ecb.csr_to_hapcsc_values_host(m.indptrA, m.indicesA, m.dataA, values, m.num_loci, m.num_haplotypes, _device(device)))
    return convert


def device_csr(parts, n_ecs, n_loci, device=None):
    """Per-haplotype CSC (indptr, indices) -> CSR(bitmask) A = sum_h 2^h M_h, on the GPU (``ecb_hapcsc_to_csr``:
    ``bin_utils.emase2ec``, ``bin_utils.py:998-1028``)."""
    from . import ecb
    cptr = np.stack([np.asarray(ip, dtype=np.int32) for ip, _ in parts])
    cidx = np.concatenate([np.asarray(ix, dtype=np.int32) for _, ix in parts])
    return ecb.hapcsc_to_csr_host(cptr, cidx, n_ecs, _device(device))


def save(h5file, m, title=None, incidence_only=True, count_2d=None, hapcsc=device_hapcsc, device=None):
    """Write :class:`alntools_amd.bin_utils.ECMatrices` ``m`` in the EMASE layout.

    ``count_2d``: ``/count`` as the group of a 2-D sparse matrix (uint32 indptr / indices / data) rather than a vector.
    The reference writes the group whenever ``apm.count`` is 2-D -- always from ``bam2emase`` (``bam_utils.py:845``: a
    ``csc_matrix`` column even for one sample) and for several samples -- and the float64 vector from ``ec2emase`` of a
    one-sample ``.bin`` (``bin_utils.py:92-93`` flattens it).  Default: group iff more than one sample.
    ``hapcsc``: the CSR -> per-haplotype CSC conversion; the device kernel unless a test passes its checker."""
    be = _backend()
    T, H, E = m.shape
    mats = hapcsc(m, device) if hapcsc is device_hapcsc else hapcsc(m)      # (``device``: the GPU that holds / held the result)
    if count_2d is None:
        count_2d = m.num_samples != 1
    if be == "tables":
        import tables
        fil = tables.Filters(complevel=1, complib='zlib')
        with tables.open_file(h5file, 'w', title=title or '') as f:
            f.set_node_attr(f.root, 'incidence_only', incidence_only)
            f.set_node_attr(f.root, 'mtype', 'csc_matrix')
            f.set_node_attr(f.root, 'shape', (T, H, E))
            for h, sp in enumerate(mats):
                g = f.create_group(f.root, 'h%d' % h, 'Sparse matrix components for Haplotype %d' % h)
                f.create_carray(g, 'indptr', obj=sp.indptr.astype('uint32'), filters=fil)
                f.create_carray(g, 'indices', obj=sp.indices.astype('uint32'), filters=fil)
                if not incidence_only:
                    f.create_carray(g, 'data', obj=sp.data.astype(float), filters=fil)
            f.create_carray(f.root, 'lengths', obj=np.asarray(m.lengths), title='Transcript Lengths', filters=fil)
            if not count_2d:
                f.create_carray(f.root, 'count', obj=m.dataN.astype(np.float64), title='Equivalence Class Counts', filters=fil)
            else:
                g = f.create_group(f.root, 'count', 'Sparse matrix components for N matrix')
                f.create_carray(g, 'indptr', obj=m.indptrN.astype('uint32'), filters=fil)
                f.create_carray(g, 'indices', obj=m.indicesN.astype('uint32'), filters=fil)
                f.create_carray(g, 'data', obj=m.dataN.astype('uint32'), filters=fil)
            f.set_node_attr(f.root, 'hname', m.hname)
            f.create_carray(f.root, 'lname', obj=np.array(m.lname), title='Locus Names', filters=fil)
            f.create_carray(f.root, 'rname', obj=np.arange(E).astype(str), title='Read Names', filters=fil)
            f.create_carray(f.root, 'sname', obj=np.array(m.sname), title='Sample Names', filters=fil)
        return
    if be == "libhdf5":
        from . import h5lite
        with h5lite.File(h5file, 'w') as f:
            f.set_attr('/', 'TITLE', (title or '').encode())
            f.set_attr('/', 'incidence_only', np.bool_(incidence_only))
            f.set_attr('/', 'mtype', b'csc_matrix')                  # bytes: the reference's loader calls .decode() on it
            f.set_attr('/', 'shape', (T, H, E))
            for h, sp in enumerate(mats):
                f.create_group('/h%d' % h)
                f.create_array('/h%d/indptr' % h, sp.indptr.astype('uint32'))
                f.create_array('/h%d/indices' % h, sp.indices.astype('uint32'))
                if not incidence_only:
                    f.create_array('/h%d/data' % h, sp.data.astype(np.float64))
            f.create_array('/lengths', np.asarray(m.lengths))
            if not count_2d:
                f.create_array('/count', m.dataN.astype(np.float64))
            else:
                f.create_group('/count')
                f.create_array('/count/indptr', m.indptrN.astype('uint32'))
                f.create_array('/count/indices', m.indicesN.astype('uint32'))
                f.create_array('/count/data', m.dataN.astype('uint32'))
            f.set_attr('/', 'hname', list(m.hname))
            f.create_array('/lname', np.array(m.lname, dtype='S'))
            f.create_array('/rname', np.arange(E).astype('S'))
            f.create_array('/sname', np.array(m.sname, dtype='S'))
        return
    import h5py
    with h5py.File(h5file, 'w') as f:
        f.attrs['incidence_only'] = incidence_only
        f.attrs['mtype'] = np.bytes_('csc_matrix')
        f.attrs['shape'] = (T, H, E)
        for h, sp in enumerate(mats):
            g = f.create_group('h%d' % h)
            g.create_dataset('indptr', data=sp.indptr.astype('uint32'), compression='gzip', compression_opts=1)
            g.create_dataset('indices', data=sp.indices.astype('uint32'), compression='gzip', compression_opts=1)
            if not incidence_only:
                g.create_dataset('data', data=sp.data.astype(float), compression='gzip', compression_opts=1)
        f.create_dataset('lengths', data=np.asarray(m.lengths))
        if not count_2d:
            f.create_dataset('count', data=m.dataN.astype(np.float64))
        else:
            g = f.create_group('count')
            g.create_dataset('indptr', data=m.indptrN.astype('uint32'))
            g.create_dataset('indices', data=m.indicesN.astype('uint32'))
            g.create_dataset('data', data=m.dataN.astype('uint32'))
        f.attrs['hname'] = [np.bytes_(x) for x in m.hname]
        f.create_dataset('lname', data=np.array(m.lname, dtype='S'))
        f.create_dataset('rname', data=np.arange(E).astype('S'))
        f.create_dataset('sname', data=np.array(m.sname, dtype='S'))


def load(h5file, csr=device_csr, device=None):
    """EMASE ``.h5`` -> :class:`ECMatrices` (the inverse of :func:`save`; ``A = sum_h 2^h * M_h``, on the GPU unless a
    test passes its checker as ``csr``)."""
    from .bin_utils import ECMatrices
    be = _backend()
    if be == "tables":
        import tables
        with tables.open_file(h5file, 'r') as f:
            T, H, E = (int(x) for x in f.get_node_attr('/', 'shape'))
            parts = [(f.get_node('/h%d' % h, 'indptr').read(), f.get_node('/h%d' % h, 'indices').read()) for h in range(H)]
            lengths = f.get_node('/', 'lengths').read()
            hname = [x.decode() if isinstance(x, bytes) else str(x) for x in f.get_node_attr('/', 'hname')]
            lname = [x.decode() if isinstance(x, bytes) else str(x) for x in f.get_node('/', 'lname').read()]
            sname = [x.decode() if isinstance(x, bytes) else str(x) for x in f.get_node('/', 'sname').read()]
            cnode = f.get_node('/', 'count')
            if isinstance(cnode, tables.Group):
                N = (cnode.indptr.read(), cnode.indices.read(), cnode.data.read())
            else:
                c = cnode.read()
                N = (np.array([0, E]), np.arange(E), c)
    elif be == "libhdf5":
        from . import h5lite
        with h5lite.File(h5file, 'r') as f:
            T, H, E = (int(x) for x in f.get_attr('/', 'shape'))
            parts = [(f.read_array('/h%d/indptr' % h), f.read_array('/h%d/indices' % h)) for h in range(H)]
            lengths = f.read_array('/lengths')
            hname = [x.decode() if isinstance(x, bytes) else str(x) for x in f.get_attr('/', 'hname')]
            lname = [x.decode() for x in f.read_array('/lname')]
            sname = [x.decode() for x in f.read_array('/sname')]
            if f.exists('/count/indptr'):
                N = (f.read_array('/count/indptr'), f.read_array('/count/indices'), f.read_array('/count/data'))
            else:
                N = (np.array([0, E]), np.arange(E), f.read_array('/count'))
    else:
        import h5py
        with h5py.File(h5file, 'r') as f:
            T, H, E = (int(x) for x in f.attrs['shape'])
            parts = [(f['h%d/indptr' % h][()], f['h%d/indices' % h][()]) for h in range(H)]
            lengths = f['lengths'][()]
            hname = [x.decode() if isinstance(x, bytes) else str(x) for x in f.attrs['hname']]
            lname = [x.decode() for x in f['lname'][()]]
            sname = [x.decode() for x in f['sname'][()]]
            if isinstance(f['count'], h5py.Group):
                N = (f['count/indptr'][()], f['count/indices'][()], f['count/data'][()])
            else:
                N = (np.array([0, E]), np.arange(E), f['count'][()])
    a_ptr, a_idx, a_dat = csr(parts, E, T, device) if csr is device_csr else csr(parts, E, T)
    return ECMatrices(hname, lname, lengths, sname, a_ptr, a_idx, np.asarray(a_dat).astype(np.int64),
                      np.asarray(N[0]).astype(np.int64), np.asarray(N[1]).astype(np.int64), np.asarray(N[2]).astype(np.int64))


def load_values(h5file):
    """EMASE ``.h5`` written with ``incidence_only=False`` -> per haplotype ``(indptr, indices, data)`` as the file holds them (uint32,
    uint32, float64): the values :func:`save` stored, bit for bit."""
    be = _backend()
    if be == "tables":
        import tables
        with tables.open_file(h5file, 'r') as f:
            H = int(f.get_node_attr('/', 'shape')[1])
            return [tuple(f.get_node('/h%d' % h, n).read() for n in ('indptr', 'indices', 'data')) for h in range(H)]
    if be == "libhdf5":
        from . import h5lite
        with h5lite.File(h5file, 'r') as f:
            H = int(f.get_attr('/', 'shape')[1])
            return [tuple(f.read_array('/h%d/%s' % (h, n)) for n in ('indptr', 'indices', 'data')) for h in range(H)]
    import h5py
    with h5py.File(h5file, 'r') as f:
        H = int(f.attrs['shape'][1])
        return [tuple(f['h%d/%s' % (h, n)][()] for n in ('indptr', 'indices', 'data')) for h in range(H)]


def scipy_hapcsc(m):
    """CHECKER for tests (scipy on the host): what :func:`device_hapcsc` must produce."""
    return [m.haplotype_csc(h) for h in range(m.num_haplotypes)]


def scipy_csr(parts, n_ecs, n_loci):
    """CHECKER for tests (scipy on the host): what :func:`device_csr` must produce."""
    from scipy.sparse import csc_matrix
    a = None
    for h, (ip, ix) in enumerate(parts):
        mh = csc_matrix((np.full(len(ix), float(2 ** h)), np.asarray(ix).astype(int), np.asarray(ip).astype(int)), shape=(n_ecs, n_loci))
        a = mh if a is None else a + mh
    a = a.tocsr()
    a.sort_indices()
    return a.indptr, a.indices, a.data.astype(np.int64)
