"""What is done with picked power (the reference's ``src/impdar/lib/analysis/``): the geometric power correction, the
empirical attenuation framework of Hills et al. (2020) and the Kirchhoff bed roughness.  The modules, functions,
signatures and defaults are the reference's; ``continuity_index`` lives with picking (``RadarData.continuity_index``)."""
