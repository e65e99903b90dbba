"""ctypes binding of libos2s_hip.so, driven by the C ABI declared in include/os2s.h.

The header is the only place a signature is written. The first lib() parses every os2s_* declaration in it,
maps its types onto ctypes through the fixed tables _ARGTYPES / _RESTYPES (a type not in them raises) and binds
each entry point as a private function object, the attribute of the same name of the namespace C:

  _lib.C.os2s_conv1d_fwd_ws(stream, ...)

The launches -- the entry points that take an os2s_stream_t and return int -- raise Os2sError on a non-zero
status themselves (an errcheck); every other entry point returns its value, which its caller checks where it is
a status. The attributes of the CDLL object itself (lib().os2s_*) get the same signatures without the errcheck;
tests and tools may rebind those, C is not affected.

There is no CPU fallback: if the HIP library is missing this raises, loudly.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libos2s_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "os2s.h")

_lib = None

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_float = ctypes.c_float

_ARGTYPES = {
    "int": c_int, "int32_t": c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
    "unsigned long long": ctypes.c_uint64, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
    "float": c_float, "double": ctypes.c_double, "os2s_stream_t": c_void_p,
}
_RESTYPES = {
    "int": c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "uint32_t": ctypes.c_uint32,
    "const char*": ctypes.c_char_p, "void": None,
}


class Os2sError(RuntimeError):
  pass


def strip_comments(text):
  """C source without its comments and preprocessor lines."""
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  text = re.sub(r"//[^\n]*", " ", text)
  return re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)


def _norm(decl):
  return " ".join(decl.replace("*", " * ").split()).replace(" *", "*")


def _param_type(param):
  """The type of one parameter declaration ('const float* x', 'unsigned long long seed', 'int')."""
  t = _norm(param)
  if "*" in t:     # any pointer; char* alone is a string
    return ctypes.c_char_p if re.match(r"^(const )?char\*( \w+)?$", t) else c_void_p
  t = re.sub(r"^const ", "", t)
  for name in (t, t.rsplit(" ", 1)[0]):
    if name in _ARGTYPES:
      return _ARGTYPES[name]
  raise Os2sError("os2s.h: no ctypes mapping for the parameter %r" % param)


def declarations(path=HEADER):
  """{name: (restype, argtypes, is_launch)} of every os2s_* function the header declares; is_launch: returns
  int and takes an os2s_stream_t (its result is an OS2S_OK / OS2S_ERR_* status)."""
  text = strip_comments(open(path).read())
  out = {}
  for m in re.finditer(r"([\w\s*]+?)\b(os2s_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
    ret, name, params = _norm(m.group(1)), m.group(2), m.group(3).strip()
    if ret not in _RESTYPES:
      raise Os2sError("os2s.h: no ctypes mapping for the return type %r of %s" % (ret, name))
    params = [] if params in ("", "void") else params.split(",")
    is_launch = ret == "int" and any(_norm(p).split(" ")[0] == "os2s_stream_t" for p in params)
    out[name] = (_RESTYPES[ret], tuple(_param_type(p) for p in params), is_launch)
  return out


def _status(code, func, args):
  """errcheck of the launches."""
  if code:
    check(code, func.__name__)
  return code


class _EntryPoints(object):
  """C: the entry points bound from the header; the first attribute read loads the library."""

  def __getattr__(self, name):
    if _lib is None:
      lib()
      return getattr(self, name)
    raise AttributeError("%s is not declared in include/os2s.h" % name)


C = _EntryPoints()


def lib():
  """Returns the loaded shared library (loads it and binds C on first use)."""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise Os2sError(
          "libos2s_hip.so not found at %s. Build it with "
          "`python -c 'import __graft_entry__ as g; g.build()'` "
          "(there is no CPU fallback for the HIP path)." % LIB_PATH)
    # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so). Device
    # pointers and streams are only valid inside ONE runtime instance, so make
    # sure torch's copy is the one already mapped (same soname) before our
    # library, which links libamdhip64.so.7, is loaded.
    import torch  # noqa: F401
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tlib):
      ctypes.CDLL(tlib, mode=ctypes.RTLD_GLOBAL)
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes, is_launch) in declarations().items():
      raw, own = getattr(L, name), L[name]       # L[name] is a fresh object, not the cached attribute
      raw.restype = own.restype = restype
      raw.argtypes = own.argtypes = argtypes
      if is_launch:
        own.errcheck = _status
      C.__dict__[name] = own
    _lib = L
  return _lib


def check(code, what=""):
  if code != 0:
    msg = C.os2s_strerror(int(code)).decode()
    detail = C.os2s_last_error_detail().decode()
    if detail:
      msg += " [" + detail + "]"
    raise Os2sError("%s failed: %s (code %d)" % (what or "os2s call", msg, code))


def bind(name, argtypes, restype=c_int):
  """Returns the library's own attribute `name` with the signature given by hand (tests that bind an entry point
  the way a plain-ctypes user would); the package calls C, which this does not touch."""
  f = getattr(lib(), name)
  f.argtypes = argtypes
  f.restype = restype
  return f


def set_option(name, value):
  """os2s_set_option: the library's named test / measurement options (include/os2s.h lists them)."""
  if C.os2s_set_option(name.encode(), float(value)) != 0:
    raise Os2sError("os2s_set_option: unknown option %r" % (name,))


def get_option(name):
  """os2s_get_option: the value the launch path reads for a named option."""
  v = ctypes.c_double()
  if C.os2s_get_option(name.encode(), ctypes.byref(v)) != 0:
    raise Os2sError("os2s_get_option: unknown option %r" % (name,))
  return v.value


def option_names():
  out, i = [], 0
  while True:
    n = C.os2s_option_name(i)
    if n is None:
      return out
    out.append(n.decode())
    i += 1


def set_debug_stamps(kernel, ptr, mode=0):
  """os2s_set_debug_stamps: device buffer (address or None) an instrumented kernel writes time stamps into."""
  if C.os2s_set_debug_stamps(kernel.encode(), c_void_p(int(ptr) if ptr else 0), int(mode)) != 0:
    raise Os2sError("os2s_set_debug_stamps: unknown kernel %r" % (kernel,))
