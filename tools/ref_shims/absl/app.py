def run(main, argv=None):
  raise RuntimeError('absl.app shim: the reference scripts are imported, not run')
